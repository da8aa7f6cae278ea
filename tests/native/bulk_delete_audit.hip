// Audit of a flat index's device arrays and derived copies after bulk deletes (GpuFlatIndex::remove_bulk; test tool, not
// shipped; driven by tests/test_gpu_bulk_delete_audit.py).
//
//   bulk_delete_audit a          a scripted stream at dim 100: holes at the edges of the index, of a 16-row fragment group and
//                                of a 64-row tile, below some watermarks and above others, repeated / absent / triple ids
//   bulk_delete_audit b [seed]   a seeded random stream at dim 128 (3000 rows, bulk deletes of every size, rows added between)
//
// Both run with the delete compaction buffer at 16 KiB, so that delete_plan.hpp cuts every array into many segments of both
// kinds.  The program keeps a plain host mirror (ids and f64 rows; a bulk delete erases every row whose id is in the list,
// order preserved) and takes a CHECKPOINT after every bulk delete: the mirror's rows are uploaded to a scratch master and
// converted from row 0 by the library's own launchers; the index must equal that from-scratch state, byte for byte:
//   - len(), the exported ids and master bits;
//   - the f32 slab (padding columns included), inv_norm, the device flags, the host row flags, the out-of-domain count;
//   - every watermark (slab16_rows_, slab16f_rows_, slab8_rows_, d_ids_rows_) is at or below the smallest removed position
//     (and below every position touched since the copy was last built); below its watermark each lazily built copy equals
//     the fresh conversion; then the copies the checkpoint's schedule names are built (ensure_*), must have their watermark
//     at n and equal the fresh conversion everywhere.  Only some copies are built at a time, so the watermarks diverge.
// One line per failed comparison, then "audit ok" or "audit FAILED" (exit status 1).  The stream stops at the first failing
// checkpoint.
#include "../../vectorlite_amd/csrc/flat_index.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_set>
#include <vector>

namespace vl {

// The peer flat_index.hpp names as a friend of GpuFlatIndex: this program's own definition of it.
class DerivedCopiesProbe {
public:
    explicit DerivedCopiesProbe(const GpuFlatIndex* index) : ix(index) {}
    const GpuFlatIndex* ix;

    const float* slab() const { return ix->d_slab_; }
    const float* inv_norm() const { return ix->d_inv_norm_; }
    const uint8_t* flags() const { return ix->d_flags_; }
    const void* slab16() const { return ix->d_slab16_; }
    const void* slab16f() const { return ix->d_slab16f_; }
    const float* norm16() const { return ix->d_norm16_; }
    const float* sqnorm() const { return ix->d_sqnorm_; }
    const void* slab8() const { return ix->d_slab8_; }
    const float* sr8() const { return ix->d_sr8_; }
    const float* norm8() const { return ix->d_norm8_; }
    const unsigned long long* dev_ids() const { return ix->d_ids_; }
    uint64_t dev_ids_cap() const { return ix->d_ids_cap_; }
    uint64_t watermark(int copy) const
    {
        const uint64_t w[4] = {ix->slab16_rows_, ix->slab16f_rows_, ix->slab8_rows_, ix->d_ids_rows_};
        return w[copy];
    }
    const std::vector<uint8_t>& row_flags() const { return ix->row_flags_; }
    uint64_t n_out_of_domain() const { return ix->n_out_of_domain_; }
    uint64_t mutations() const { return ix->mutations_; }
    int ensure(int copy) const  // the lazy builds, called as the search routes call them: under the shared index lock
    {
        std::shared_lock<RwLock> lk(ix->mu_);
        if (hipSetDevice(ix->device_) != hipSuccess) return ERR_DEVICE;
        switch (copy) {
        case 0: return ix->ensure_bf16_slab(false);
        case 1: return ix->ensure_bf16_slab(true);
        case 2: return ix->ensure_i8_slab();
        default: return ix->ensure_device_ids();
        }
    }
};

}  // namespace vl

using namespace vl;

namespace {

#define CK(x)                                                                                  \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) {                                                                \
            printf("FAIL %s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));       \
            printf("audit FAILED\n");                                                          \
            exit(1);                                                                           \
        }                                                                                      \
    } while (0)

enum Copy : int { C_ROW = 0, C_FRAG = 1, C_I8 = 2, C_IDS = 3 };
constexpr int M_ROW = 1, M_FRAG = 2, M_I8 = 4, M_IDS = 8, M_ALL = 15;
const char* const COPY_NAME[4] = {"slab16_rows_", "slab16f_rows_", "slab8_rows_", "d_ids_rows_"};
constexpr uint64_t BOUNCE = 16 << 10;

uint64_t splitmix(uint64_t& x)
{
    uint64_t z = (x += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
double uniform01(uint64_t& x) { return ((double)(splitmix(x) >> 11) + 0.5) * 0x1.0p-53; }
double normal(uint64_t& x) { return std::sqrt(-2.0 * std::log(uniform01(x))) * std::cos(6.283185307179586 * uniform01(x)); }

// a gaussian direction at norm 0.25, 1 or 4 times a per-row factor: every row differs from its neighbours in every per-row
// array, so an entry shifted by one row differs in its bytes.  Every 97th row lies outside the fast path's domain (a value
// of 2^41), so that the flags and the out-of-domain count have something to lose.
void random_row(uint64_t& rng, uint32_t dim, uint64_t serial, double* out)
{
    double ss = 0.0;
    for (uint32_t c = 0; c < dim; ++c) {
        out[c] = normal(rng);
        ss += out[c] * out[c];
    }
    const double scales[3] = {0.25, 1.0, 4.0};
    const double f = scales[splitmix(rng) % 3] * (1.0 + 0.0625 * uniform01(rng)) / std::sqrt(ss);
    for (uint32_t c = 0; c < dim; ++c) out[c] *= f;
    if (serial % 97 == 96) out[serial % dim] = 2199023255552.0;
}

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    T* need(size_t count)
    {
        if (count > cap) {
            if (p) CK(hipFree(p));
            cap = count + count / 2 + 64;
            CK(hipMalloc(reinterpret_cast<void**>(&p), cap * sizeof(T)));
        }
        return p;
    }
    ~DevBuf()
    {
        if (p) (void)hipFree(p);
    }
};

template <typename T>
std::vector<T> download(const T* d, size_t count)
{
    std::vector<T> h(count);
    if (count) CK(hipMemcpy(h.data(), d, count * sizeof(T), hipMemcpyDeviceToHost));
    return h;
}

struct Fresh {  // the from-scratch state of n rows
    std::vector<float> slab, inv, n16, sq, sr8, n8;
    std::vector<uint8_t> flags, b8;
    std::vector<uint16_t> b16;
};

struct Audit {
    uint32_t dim, ld, ldb;
    bool frag_ok;
    GpuFlatIndex* ix = nullptr;
    std::vector<uint64_t> ids;  // the mirror
    std::vector<double> rows;
    uint64_t bound[4] = {0, 0, 0, 0};  // per copy: rows it held when last built, lowered to every position touched since
    uint64_t next_serial = 0;
    bool failed = false;
    int ckpt = 0;
    std::string op = "start";
    hipStream_t stream = nullptr;
    DevBuf<double> s_master;
    DevBuf<float> s_slab, s_inv, s_n16, s_sq, s_sr8, s_n8;
    DevBuf<uint8_t> s_flags, s_b8;
    DevBuf<uint16_t> s_b16;
    DevBuf<IngestStats> s_stats;

    explicit Audit(uint32_t d) : dim(d), ld((d + 3u) & ~3u), ldb(mfma_ldb(d))
    {
        frag_ok = mfma_rows_kernel(d) && ldb % 32 == 0;
        CK(hipStreamCreate(&stream));
        if (GpuFlatIndex::create(d, 0, &ix) != OK) die("create");
        if (ix->set_delete_bounce(BOUNCE) != OK) die("set_delete_bounce");
    }
    ~Audit()
    {
        delete ix;
        (void)hipStreamDestroy(stream);
    }
    [[noreturn]] void die(const char* what)
    {
        printf("FAIL %s: %s\n", what, last_error());
        printf("audit FAILED\n");
        exit(1);
    }
    uint64_t n() const { return ids.size(); }
    void fail(const char* array, long long row, long long col, const std::string& note = "")
    {
        printf("FAIL %s checkpoint %d op [%s] row %lld col %lld%s%s\n", array, ckpt, op.c_str(), row, col, note.empty() ? "" : " ",
               note.c_str());
        failed = true;
    }
    bool same(const char* array, const void* got, const void* want, size_t n_rows, size_t row_elems, size_t elem)
    {
        const size_t total = n_rows * row_elems * elem;
        if (total == 0 || memcmp(got, want, total) == 0) return true;
        const unsigned char* a = static_cast<const unsigned char*>(got);
        const unsigned char* b = static_cast<const unsigned char*>(want);
        size_t i = 0;
        while (a[i] == b[i]) ++i;
        const size_t e = i / elem;
        fail(array, (long long)(e / row_elems), (long long)(e % row_elems));
        return false;
    }

    Fresh convert()
    {
        Fresh f;
        const size_t m = n();
        if (m == 0) return f;
        CK(hipMemcpy(s_master.need(m * dim), rows.data(), m * dim * sizeof(double), hipMemcpyHostToDevice));
        CK(hipMemsetAsync(s_stats.need(1), 0, sizeof(IngestStats), stream));
        CK(launch_ingest(stream, s_master.p, s_slab.need(m * ld), s_inv.need(m), s_flags.need(m), s_stats.p, m, dim, ld));
        CK(launch_rows_bf16(stream, s_master.p, m, dim, s_b16.need(m * ldb), s_n16.need(m), s_sq.need(m)));
        CK(launch_rows_i8(stream, s_master.p, m, dim, s_b8.need(m * ldb), s_sr8.need(2 * m), s_n8.need(m)));
        CK(hipStreamSynchronize(stream));
        f.slab = download(s_slab.p, m * ld);
        f.inv = download(s_inv.p, m);
        f.flags = download(s_flags.p, m);
        f.b16 = download(s_b16.p, m * ldb);
        f.n16 = download(s_n16.p, m);
        f.sq = download(s_sq.p, m);
        f.b8 = download(s_b8.p, m * ldb);
        f.sr8 = download(s_sr8.p, 2 * m);
        f.n8 = download(s_n8.p, m);
        return f;
    }

    void check_copy(const DerivedCopiesProbe& pr, const Fresh& f, int c, uint64_t w)  // one lazily built copy over its first w rows
    {
        if (w == 0) return;
        if (c == C_ROW) {
            if (!pr.slab16() || !pr.norm16()) return fail("d_slab16_", -1, -1, "null with a watermark above 0");
            same("d_slab16_", download(static_cast<const uint16_t*>(pr.slab16()), w * ldb).data(), f.b16.data(), w, ldb, 2);
        } else if (c == C_FRAG) {
            if (!pr.slab16f() || !pr.norm16()) return fail("d_slab16f_", -1, -1, "null with a watermark above 0");
            // whole 16-row groups; the offset is the one documented above k_rows_bf16_frag
            const uint64_t groups = (w + 15) / 16;
            const uint32_t ks32 = ldb / 32;
            const std::vector<unsigned char> fr = download(static_cast<const unsigned char*>(pr.slab16f()), groups * 16 * ldb * 2);
            for (uint64_t r = 0; r < w; ++r)
                for (uint32_t p = 0; p < ldb / 8; ++p) {
                    const size_t off = ((((size_t)(r >> 4) * ks32 + (p >> 2)) * 64) + (size_t)((p & 3) * 16 + (uint32_t)(r & 15))) * 16;
                    if (memcmp(&fr[off], &f.b16[r * ldb + 8 * p], 16) != 0) return fail("d_slab16f_", (long long)r, (long long)(8 * p));
                }
        } else if (c == C_I8) {
            if (!pr.slab8() || !pr.sr8() || !pr.norm8()) return fail("d_slab8_", -1, -1, "null with a watermark above 0");
            same("d_slab8_", download(static_cast<const uint8_t*>(pr.slab8()), w * ldb).data(), f.b8.data(), w, ldb, 1);
            same("d_sr8_", download(pr.sr8(), 2 * w).data(), f.sr8.data(), w, 2, 4);
            same("d_norm8_", download(pr.norm8(), w).data(), f.n8.data(), w, 1, 4);
        } else {
            if (!pr.dev_ids() || pr.dev_ids_cap() < w) return fail("d_ids_", -1, -1, "null or too small for its watermark");
            same("d_ids_", download(pr.dev_ids(), w).data(), ids.data(), w, 1, 8);
        }
    }
    void check_copies(const DerivedCopiesProbe& pr, const Fresh& f)
    {
        const uint64_t m = n();
        for (int c = 0; c < 4; ++c) check_copy(pr, f, c, std::min<uint64_t>(pr.watermark(c), m));
        const uint64_t wn = std::min<uint64_t>(std::max(pr.watermark(C_ROW), pr.watermark(C_FRAG)), m);  // shared by both bf16 copies
        if (wn && pr.norm16() && pr.sqnorm()) {
            same("d_norm16_", download(pr.norm16(), wn).data(), f.n16.data(), wn, 1, 4);
            same("d_sqnorm_", download(pr.sqnorm(), wn).data(), f.sq.data(), wn, 1, 4);
        }
    }

    // `build` names the lazy copies built at the end of this checkpoint
    void checkpoint(int build)
    {
        if (failed) return;
        ++ckpt;
        if (!frag_ok) build &= ~M_FRAG;
        const DerivedCopiesProbe pr(ix);
        const uint64_t m = n();
        if (ix->len() != m) return fail("len", (long long)ix->len(), (long long)m, "(row = len(), col = the mirror's)");
        {
            std::vector<uint64_t> eid(m);
            std::vector<double> erow(m * dim);
            if (ix->export_rows(eid.data(), erow.data()) != OK) die("export_rows");
            same("ids_", eid.data(), ids.data(), m, 1, 8);
            same("d_master_", erow.data(), rows.data(), m, dim, 8);
            if (failed) return;
        }
        const Fresh f = convert();
        same("d_slab_", download(pr.slab(), m * ld).data(), f.slab.data(), m, ld, 4);
        same("d_inv_norm_", download(pr.inv_norm(), m).data(), f.inv.data(), m, 1, 4);
        same("d_flags_", download(pr.flags(), m).data(), f.flags.data(), m, 1, 1);
        if (pr.row_flags().size() != m)
            fail("row_flags_", (long long)pr.row_flags().size(), (long long)m, "(row = its size, col = the mirror's)");
        else
            same("row_flags_", pr.row_flags().data(), f.flags.data(), m, 1, 1);
        uint64_t ood = 0;
        for (uint8_t b : f.flags) ood += (b & ROW_OUT_OF_DOMAIN) != 0;
        if (pr.n_out_of_domain() != ood) fail("n_out_of_domain_", (long long)pr.n_out_of_domain(), (long long)ood, "(row = held, col = fresh)");
        if (failed) return;
        // as the delete left them: no watermark above the smallest position touched, every copy right below its watermark
        for (int c = 0; c < 4; ++c)
            if (pr.watermark(c) > bound[c])
                fail(COPY_NAME[c], (long long)pr.watermark(c), (long long)bound[c],
                     "(row = watermark, col = smallest position touched since its last build)");
        check_copies(pr, f);
        if (failed) return;
        // built now: at n, and right everywhere
        for (int c = 0; c < 4; ++c) {
            if (!(build & (1 << c))) continue;
            if (pr.ensure(c) != OK) die("ensure");
            bound[c] = m;
            if (pr.watermark(c) != m) fail(COPY_NAME[c], (long long)pr.watermark(c), (long long)m, "(row = watermark after its build, col = n)");
        }
        check_copies(pr, f);
    }

    void add_random(uint64_t& rng, uint64_t count, uint64_t id_base, int build)
    {
        if (failed) return;
        op = "add_bulk of " + std::to_string(count) + " at n=" + std::to_string(n());
        std::vector<uint64_t> new_ids(count);
        std::vector<double> new_rows(count * dim);
        for (uint64_t i = 0; i < count; ++i) {
            new_ids[i] = id_base + i * 3;
            random_row(rng, dim, next_serial++, &new_rows[i * dim]);
        }
        if (ix->add_bulk(new_ids.data(), new_rows.data(), count, false, false) != OK) die(op.c_str());
        ids.insert(ids.end(), new_ids.begin(), new_ids.end());
        rows.insert(rows.end(), new_rows.begin(), new_rows.end());
        checkpoint(build);
    }
    // the ids stored at these positions, handed over in the order given
    std::vector<uint64_t> ids_at(const std::vector<uint64_t>& positions) const
    {
        std::vector<uint64_t> out;
        for (uint64_t p : positions) out.push_back(ids[p]);
        return out;
    }
    void remove_bulk(const std::vector<uint64_t>& list, int build, const char* what)
    {
        if (failed) return;
        const std::unordered_set<uint64_t> gone(list.begin(), list.end());
        uint64_t first = ~0ull, w = 0, hit = 0;
        for (uint64_t p = 0; p < n(); ++p) {
            if (gone.count(ids[p])) {
                if (first == ~0ull) first = p;
                ++hit;
                continue;
            }
            if (w != p) {
                ids[w] = ids[p];
                memcpy(&rows[w * dim], &rows[p * dim], dim * sizeof(double));
            }
            ++w;
        }
        op = std::string(what) + ": " + std::to_string(list.size()) + " ids, " + std::to_string(hit) + " rows from position " +
             (hit ? std::to_string(first) : std::string("none")) + " of n=" + std::to_string(n());
        ids.resize(w);
        rows.resize(w * dim);
        if (hit)
            for (uint64_t& b : bound) b = std::min(b, first);
        const uint64_t before = DerivedCopiesProbe(ix).mutations();
        std::vector<uint64_t> positions;
        uint64_t reported = ~0ull;
        if (ix->remove_bulk(list.data(), list.size(), &positions, &reported) != OK) die(op.c_str());
        if (reported != hit || positions.size() != hit || (hit && positions[0] != first) || !std::is_sorted(positions.begin(), positions.end()))
            fail("remove_bulk", (long long)reported, (long long)hit, "(row = rows reported, col = the mirror's)");
        if (DerivedCopiesProbe(ix).mutations() != before + (hit ? 1 : 0)) fail("mutations_", -1, -1, "must move once per bulk delete that removes a row");
        checkpoint(build);
    }
};

int scripted(uint32_t dim)
{
    Audit a(dim);
    uint64_t rng = 0xB01Dull + dim;
    a.add_random(rng, 2600, 1000, M_ALL);
    // a triple id (unvalidated adds accept it): positions 40, 1300 and 2599
    a.ids[40] = a.ids[1300] = a.ids[2599] = 5;
    {
        delete a.ix;
        a.ix = nullptr;
        if (GpuFlatIndex::create(dim, 0, &a.ix) != OK || a.ix->set_delete_bounce(BOUNCE) != OK) a.die("create");
        for (uint64_t& b : a.bound) b = 0;
        a.op = "rebuilt with a triple id";
        if (a.ix->add_bulk(a.ids.data(), a.rows.data(), a.n(), false, false) != OK) a.die("add_bulk");
        a.checkpoint(M_ALL);
    }
    // the edges of the index; every copy is built, so each hole lies below every watermark
    a.remove_bulk(a.ids_at({0}), M_ALL, "first row");
    a.remove_bulk(a.ids_at({a.n() - 1}), M_ALL, "last row");
    a.remove_bulk(a.ids_at({0, a.n() - 1}), M_ROW | M_IDS, "both ends");
    // the fragment-major and int8 copies now end at 0, the others at n: holes above the former, below the latter
    a.remove_bulk(a.ids_at({15, 16, 17}), M_FRAG, "around the end of fragment group 0");
    a.remove_bulk(a.ids_at({63, 64, 65, 127, 128}), M_I8, "around the ends of tiles 0 and 1");
    a.remove_bulk(a.ids_at({1024 + 15, 1024 + 16, 1024 + 63, 1024 + 64}), 0, "group and tile edges in the middle, nothing built");
    a.remove_bulk(a.ids_at({2000}), M_ALL, "one hole, then every copy built");
    a.remove_bulk({5}, M_ROW, "the triple id");
    a.remove_bulk({5, 7, 7, (uint64_t)-1}, 0, "only absent and repeated ids");
    {
        std::vector<uint64_t> l = a.ids_at({300, 31, 32, 300, 1999, 31});
        l.push_back(123456789012ull);
        a.remove_bulk(l, M_FRAG | M_I8, "repeats and an absent id, unsorted");
    }
    {
        std::vector<uint64_t> pos;
        for (uint64_t p = 640; p < 640 + 16 * 37; ++p) pos.push_back(p);  // a run from a tile edge to a group edge
        a.remove_bulk(a.ids_at(pos), M_IDS, "one long run");
        pos.clear();
        for (uint64_t p = 1; p < a.n(); p += 2) pos.push_back(p);
        a.remove_bulk(a.ids_at(pos), M_ALL, "every other row");
        a.add_random(rng, 700, 1ull << 40, M_ROW | M_I8);  // growth behind a compaction
        pos.clear();
        for (uint64_t p = a.n() - 500; p < a.n(); p += 3) pos.push_back(p);
        a.remove_bulk(a.ids_at(pos), 0, "holes among the new rows only");
        a.remove_bulk(std::vector<uint64_t>(a.ids), M_ALL, "every row");
        a.add_random(rng, 100, 1ull << 41, M_ALL);
    }
    printf("stream scripted dim=%u: %d checkpoints, n=%llu at the end\n", dim, a.ckpt, (unsigned long long)a.n());
    return a.failed ? 1 : 0;
}

int seeded(uint32_t dim, uint64_t seed)
{
    Audit a(dim);
    uint64_t rng = seed * 0x9E3779B97F4A7C15ull + 77;
    a.add_random(rng, 3000, 1000, M_ALL);
    uint64_t id_base = 1ull << 40;
    for (int round = 0; round < 24 && !a.failed; ++round) {
        const uint64_t m = a.n();
        std::vector<uint64_t> list;
        const int kind = (int)(splitmix(rng) % 6);
        if (m == 0) {
            list.push_back(42);
        } else if (kind == 0) {
            list.push_back(a.ids[splitmix(rng) % m]);
        } else if (kind == 1) {  // a contiguous run
            const uint64_t start = splitmix(rng) % m, len = 1 + splitmix(rng) % std::min<uint64_t>(m - start, 400);
            for (uint64_t p = start; p < start + len; ++p) list.push_back(a.ids[p]);
        } else {  // a random share: about 1, 5, 15 or 40 per cent
            const double share[4] = {0.01, 0.05, 0.15, 0.40};
            for (uint64_t p = 0; p < m; ++p)
                if (uniform01(rng) < share[kind - 2]) list.push_back(a.ids[p]);
        }
        for (int j = 0; j < 3; ++j) list.push_back(7 + splitmix(rng) % 900);            // absent (stored ids start at 1000)
        for (size_t j = 0, e = list.size(); j < e && j < 5; ++j) list.push_back(list[j]);  // named twice
        for (size_t j = list.size(); j > 1; --j) std::swap(list[j - 1], list[splitmix(rng) % j]);
        a.remove_bulk(list, (int)(splitmix(rng) % 16), "seeded bulk delete");
        if (round % 4 == 3 || a.n() < 600) {
            a.add_random(rng, 300 + splitmix(rng) % 500, id_base, (int)(splitmix(rng) % 16));
            id_base += 1ull << 20;
        }
    }
    printf("stream seeded dim=%u seed=%llu: %d checkpoints, n=%llu at the end\n", dim, (unsigned long long)seed, a.ckpt,
           (unsigned long long)a.n());
    return a.failed ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "a";
    int bad = 0;
    if (mode == "a") bad = scripted(100);
    else if (mode == "b") bad = seeded(128, argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
    else {
        printf("usage: bulk_delete_audit a | b [seed]\n");
        return 2;
    }
    fputs(bad ? "audit FAILED\n" : "audit ok\n", stdout);
    return bad;
}
