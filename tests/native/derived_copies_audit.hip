// Audit of every device copy a flat index derives from its f64 master rows, after streams of adds, deletes and truncates
// (test tool, not shipped; driven by tests/test_gpu_derived_copies.py).
//
//   derived_copies_audit a          watermarks and boundaries: a scripted stream at dim 100 and dim 384
//   derived_copies_audit b [seed]   a seeded random stream at dim 128 (3000 rows, 150 operations)
//   derived_copies_audit c          the delete's bounce loop: 9000 rows of dim 1000, a move of more than one 64 MB chunk
//
// The program keeps a plain host mirror of the index (ids and f64 rows: append on add, order-preserving erase of every row
// with the id on delete, resize on truncate) and, after every mutation, takes a CHECKPOINT: the mirror's rows are uploaded
// to a scratch master and converted from row 0 by the library's own launchers (launch_ingest, launch_rows_bf16,
// launch_rows_i8); the index's incremental state must equal that from-scratch state, byte for byte:
//   - len(), the exported ids and master bits;
//   - the f32 slab (padding columns included), inv_norm, the device flags, the host row flags, the out-of-domain count;
//     the largest row norm may stay high after a delete or truncate and is exact on an index that had neither;
//   - the lazily built copies (row-major bf16, fragment-major bf16 with the two per-row arrays they share, int8 with its
//     (s, r) pairs and norms, the device id table).  Each checkpoint builds only the copies its schedule names, so the four
//     watermarks diverge and deletes land below some and above others.  A copy built now has its watermark at n and equals
//     the fresh copy everywhere; a copy not built now has its watermark at or below the smallest position touched since it
//     was last built, and equals the fresh copy below that watermark;
//   - two id filters and a group table kept alive through the stream, resolved again through resolve_if_stale: the
//     position lists and group_of_row[] equal what the mirror gives.
// One line per failed comparison (array, checkpoint, operation, first differing row and column), then "audit ok" or
// "audit FAILED" (exit status 1).  The stream stops at the first failing checkpoint.
//
// The conversion kernels' own correctness is the business of filter_audit.hip and filter_audit_i8.hip.
#include "../../vectorlite_amd/csrc/flat_index.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace vl {

// The peer flat_index.hpp names as a friend of GpuFlatIndex: everything the audit reads that has no public accessor.
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
    double max_row_norm() const { return ix->max_row_norm_; }
    uint64_t mutations() const { return ix->mutations_; }
    uint32_t ld() const { return ix->ld_; }

    // the lazy builds, called as the search routes call them: under the shared index lock
    int ensure(int copy) const
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
    // what run_search does with a search's filter and group table before its body runs
    template <typename T>
    int resolve(T* target) const
    {
        std::shared_lock<RwLock> lk(ix->mu_);
        if (hipSetDevice(ix->device_) != hipSuccess) return ERR_DEVICE;
        Workspace* ws = ix->acquire_ws();
        if (!ws) return ERR_DEVICE;
        const int rc = ix->resolve_if_stale(ws, target);
        (void)hipStreamSynchronize(ws->stream);
        ix->release_ws(ws);
        return rc;
    }
    int filter(uint64_t token, std::shared_ptr<IdFilter>* out) const { return ix->find_filter(token, out); }
    int groups(uint64_t token, std::shared_ptr<GroupTable>* out) const { return ix->find_groups(token, out); }
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

uint64_t splitmix(uint64_t& x)
{
    uint64_t z = (x += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
double uniform01(uint64_t& x) { return ((double)(splitmix(x) >> 11) + 0.5) * 0x1.0p-53; }
double normal(uint64_t& x) { return std::sqrt(-2.0 * std::log(uniform01(x))) * std::cos(6.283185307179586 * uniform01(x)); }

// a gaussian direction at norm 0.25, 1 or 4, times a per-row factor in [1, 1 + 2^-4) without which two rows of one
// magnitude would share their f32 norm: every row differs from its neighbours in every per-row array (inv_norm, norm16,
// sqnorm, the int8 pair and norm), so an entry shifted by one row differs in its bytes
void random_row(uint64_t& rng, uint32_t dim, double* out)
{
    double ss = 0.0;
    for (uint32_t c = 0; c < dim; ++c) {
        out[c] = normal(rng);
        ss += out[c] * out[c];
    }
    const double scales[3] = {0.25, 1.0, 4.0};
    const double f = scales[splitmix(rng) % 3] * (1.0 + 0.0625 * uniform01(rng)) / std::sqrt(ss);
    for (uint32_t c = 0; c < dim; ++c) out[c] *= f;
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

// the from-scratch state of n rows
struct Fresh {
    std::vector<float> slab, inv, n16, sq, sr8, n8;
    std::vector<uint8_t> flags, b8;
    std::vector<uint16_t> b16;
    uint64_t n_ood = 0;
    double max_norm = 0.0;
};

struct Audit {
    uint32_t dim, ld, ldb;
    bool frag_ok;  // the fragment-major copy exists for this dimension (the row-stationary MFMA kernel's strides)
    GpuFlatIndex* ix = nullptr;
    std::vector<uint64_t> ids;   // the mirror
    std::vector<double> rows;
    uint64_t bound[4] = {0, 0, 0, 0};  // per copy: rows it held when last built, lowered to every position touched since
    bool shrunk = false;               // a delete or truncate happened: max_row_norm_ may stay high
    bool failed = false;
    int ckpt = 0;
    std::string op = "start";
    hipStream_t stream = nullptr;
    DevBuf<double> s_master;
    DevBuf<float> s_slab, s_inv, s_n16, s_sq, s_sr8, s_n8;
    DevBuf<uint8_t> s_flags, s_b8;
    DevBuf<uint16_t> s_b16;
    DevBuf<IngestStats> s_stats;
    // the filters and the group table that live through the stream: the caller's ids / pairs, kept to create them again
    // on a clone and to compute what the mirror expects
    std::vector<uint64_t> fset[2];  // sorted
    uint64_t ftoken[2] = {0, 0};
    std::vector<uint64_t> g_ids, g_keys;
    GroupPlan plan;
    uint64_t gtoken = 0;

    Audit(uint32_t d) : dim(d), ld((d + 3u) & ~3u), ldb(mfma_ldb(d))
    {
        frag_ok = mfma_rows_kernel(d) && ldb % 32 == 0;
        CK(hipStreamCreate(&stream));
        if (GpuFlatIndex::create(d, 0, &ix) != OK) die("create");
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
    // rows x row_elems elements of elem bytes each: the first differing element
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

    // ---- the mirror's rows converted from row 0 ----
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
        const IngestStats st = download(s_stats.p, 1)[0];
        f.n_ood = st.n_out_of_domain;
        memcpy(&f.max_norm, &st.max_norm_bits, 8);
        return f;
    }

    // ---- one lazily built copy over its first w rows ----
    void check_copy(const DerivedCopiesProbe& pr, const Fresh& f, int c, uint64_t w)
    {
        if (w == 0) return;
        if (c == C_ROW) {
            if (!pr.slab16() || !pr.norm16()) return fail("d_slab16_", -1, -1, "null with a watermark above 0");
            same("d_slab16_", download(static_cast<const uint16_t*>(pr.slab16()), w * ldb).data(), f.b16.data(), w, ldb, 2);
        } else if (c == C_FRAG) {
            if (!pr.slab16f() || !pr.norm16()) return fail("d_slab16f_", -1, -1, "null with a watermark above 0");
            // whole 16-row groups (the allocation is in whole 64-row tiles); the offset is the one documented above k_rows_bf16_frag
            const uint64_t groups = (w + 15) / 16;
            const uint32_t ks32 = ldb / 32;
            const std::vector<unsigned char> fr = download(static_cast<const unsigned char*>(pr.slab16f()), groups * 16 * ldb * 2);
            for (uint64_t r = 0; r < w; ++r)
                for (uint32_t p = 0; p < ldb / 8; ++p) {
                    const size_t off = ((((size_t)(r >> 4) * ks32 + (p >> 2)) * 64) + (size_t)((p & 3) * 16 + (uint32_t)(r & 15))) * 16;
                    const uint16_t* want = &f.b16[r * ldb + 8 * p];
                    if (memcmp(&fr[off], want, 16) != 0) {
                        uint16_t got[8];
                        memcpy(got, &fr[off], 16);
                        int e = 0;
                        while (got[e] == want[e]) ++e;
                        return fail("d_slab16f_", (long long)r, (long long)(8 * p + e));
                    }
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

    void check_resolved(const DerivedCopiesProbe& pr)
    {
        const uint64_t m = n();
        for (int i = 0; i < 2 && !failed; ++i) {
            std::shared_ptr<IdFilter> fl;
            if (pr.filter(ftoken[i], &fl) != OK) die("find_filter");
            if (pr.resolve(fl.get()) != OK) die("resolve_if_stale(filter)");
            const char* name = i ? "filter B d_plist" : "filter A d_plist";
            std::vector<uint32_t> want;
            for (uint64_t p = 0; p < m; ++p)
                if (std::binary_search(fset[i].begin(), fset[i].end(), ids[p])) want.push_back((uint32_t)p);
            uint64_t reported = ~0ull;
            if (ix->filter_rows(ftoken[i], &reported) != OK) die("filter_rows");
            if (fl->resolved_at != pr.mutations()) fail(name, -1, -1, "resolved_at is not the mutation count");
            if (fl->m != want.size() || reported != want.size())
                fail(name, (long long)fl->m, (long long)want.size(), "(row = rows resolved, col = rows expected)");
            else if (!want.empty())
                same(name, download(fl->d_plist, want.size()).data(), want.data(), want.size(), 1, 4);
        }
        if (failed) return;
        std::shared_ptr<GroupTable> t;
        if (pr.groups(gtoken, &t) != OK) die("find_groups");
        if (pr.resolve(t.get()) != OK) die("resolve_if_stale(groups)");
        std::vector<uint32_t> want_rows, want_gor(m, GROUP_NONE);
        for (uint64_t p = 0; p < m; ++p) {
            const auto it = std::lower_bound(plan.ids.begin(), plan.ids.end(), ids[p]);
            if (it != plan.ids.end() && *it == ids[p]) {
                want_rows.push_back((uint32_t)p);
                want_gor[p] = plan.dense[it - plan.ids.begin()];
            }
        }
        uint64_t reported = ~0ull, distinct = ~0ull;
        if (ix->groups_rows(gtoken, &reported, &distinct) != OK) die("groups_rows");
        if (t->rows.resolved_at != pr.mutations()) fail("group table", -1, -1, "resolved_at is not the mutation count");
        if (distinct != plan.keys.size()) fail("group table keys", (long long)distinct, (long long)plan.keys.size());
        if (t->rows.m != want_rows.size() || reported != want_rows.size())
            fail("group table d_plist", (long long)t->rows.m, (long long)want_rows.size(), "(row = rows resolved, col = rows expected)");
        else if (!want_rows.empty())
            same("group table d_plist", download(t->rows.d_plist, want_rows.size()).data(), want_rows.data(), want_rows.size(), 1, 4);
        if (m && !plan.ids.empty()) {
            if (!t->d_group_of_row || t->gor_cap < m) return fail("d_group_of_row", -1, -1, "null or too small");
            same("d_group_of_row", download(t->d_group_of_row, m).data(), want_gor.data(), m, 1, 4);
        }
    }

    // ---- a checkpoint: `build` names the lazy copies built now ----
    void checkpoint(int build)
    {
        if (failed) return;
        ++ckpt;
        if (!frag_ok) build &= ~M_FRAG;
        const DerivedCopiesProbe pr(ix);
        const uint64_t m = n();
        // size and master
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
        // ingest outputs
        same("d_slab_", download(pr.slab(), m * ld).data(), f.slab.data(), m, ld, 4);
        same("d_inv_norm_", download(pr.inv_norm(), m).data(), f.inv.data(), m, 1, 4);
        same("d_flags_", download(pr.flags(), m).data(), f.flags.data(), m, 1, 1);
        if (pr.row_flags().size() != m)
            fail("row_flags_", (long long)pr.row_flags().size(), (long long)m, "(row = its size, col = the mirror's)");
        else
            same("row_flags_", pr.row_flags().data(), f.flags.data(), m, 1, 1);
        uint64_t ood = 0;
        for (uint8_t b : f.flags) ood += (b & ROW_OUT_OF_DOMAIN) != 0;
        if (ood != f.n_ood) fail("fresh ingest statistics", (long long)f.n_ood, (long long)ood);
        if (pr.n_out_of_domain() != ood) fail("n_out_of_domain_", (long long)pr.n_out_of_domain(), (long long)ood, "(row = held, col = fresh)");
        if (!(pr.max_row_norm() >= f.max_norm) || (!shrunk && pr.max_row_norm() != f.max_norm)) {
            char note[96];
            snprintf(note, sizeof note, "held %.17g fresh %.17g%s", pr.max_row_norm(), f.max_norm, shrunk ? "" : " (no delete or truncate so far)");
            fail("max_row_norm_", -1, -1, note);
        }
        if (failed) return;
        // lazy copies
        for (int c = 0; c < 4; ++c) {
            if (build & (1 << c)) {
                if (pr.ensure(c) != OK) die("ensure");
                bound[c] = m;
                if (pr.watermark(c) != m) fail(COPY_NAME[c], (long long)pr.watermark(c), (long long)m, "(row = watermark after its build, col = n)");
            } else if (pr.watermark(c) > bound[c]) {
                fail(COPY_NAME[c], (long long)pr.watermark(c), (long long)bound[c],
                     "(row = watermark, col = smallest position touched since its last build)");
            }
        }
        // the contents are compared below the watermark the index itself goes by, whatever the test above said of it
        for (int c = 0; c < 4; ++c) check_copy(pr, f, c, std::min<uint64_t>(pr.watermark(c), m));
        const uint64_t wn = std::min<uint64_t>(std::max(pr.watermark(C_ROW), pr.watermark(C_FRAG)), m);  // shared by both bf16 copies
        if (wn && pr.norm16() && pr.sqnorm()) {
            same("d_norm16_", download(pr.norm16(), wn).data(), f.n16.data(), wn, 1, 4);
            same("d_sqnorm_", download(pr.sqnorm(), wn).data(), f.sq.data(), wn, 1, 4);
        }
        if (failed) return;
        // filters and the group table; their resolution uploads the id table as far as n
        check_resolved(pr);
        if (failed) return;
        if (m) {
            bound[C_IDS] = m;
            if (pr.watermark(C_IDS) != m) fail(COPY_NAME[C_IDS], (long long)pr.watermark(C_IDS), (long long)m, "(row = watermark after a resolution, col = n)");
            check_copy(pr, f, C_IDS, std::min<uint64_t>(pr.watermark(C_IDS), m));
        }
    }

    // ---- the filters ----
    void create_filters()
    {
        for (int i = 0; i < 2; ++i) {
            std::vector<uint64_t> shuffled(fset[i].rbegin(), fset[i].rend());  // the library sorts; hand them over unsorted, with a repeat
            if (!shuffled.empty()) shuffled.push_back(shuffled[0]);
            if (ix->filter_create(shuffled.data(), shuffled.size(), &ftoken[i], nullptr) != OK) die("filter_create");
        }
        GroupPlan p;
        if (!group_plan_build(g_ids.data(), g_keys.data(), g_ids.size(), &p) || !group_plan_build(g_ids.data(), g_keys.data(), g_ids.size(), &plan))
            die("group_plan_build");
        if (ix->groups_create(std::move(p), &gtoken, nullptr) != OK) die("groups_create");
        bound[C_IDS] = n();  // the first resolution uploaded the id table
    }
    void set_filters(std::vector<uint64_t> a, std::vector<uint64_t> b, std::vector<uint64_t> gi, std::vector<uint64_t> gk)
    {
        std::sort(a.begin(), a.end());
        std::sort(b.begin(), b.end());
        fset[0] = std::move(a);
        fset[1] = std::move(b);
        g_ids = std::move(gi);
        g_keys = std::move(gk);
        create_filters();
    }

    // ---- mutations, applied to the index and to the mirror ----
    void touched(uint64_t pos)
    {
        for (uint64_t& b : bound) b = std::min(b, pos);
        shrunk = true;
    }
    void add_bulk(const std::vector<uint64_t>& new_ids, const std::vector<double>& new_rows, bool validate, int build, const char* what)
    {
        if (failed) return;
        op = std::string(what) + " of " + std::to_string(new_ids.size()) + " at n=" + std::to_string(n());
        if (ix->add_bulk(new_ids.data(), new_rows.data(), new_ids.size(), validate, false) != OK) die(op.c_str());
        ids.insert(ids.end(), new_ids.begin(), new_ids.end());
        rows.insert(rows.end(), new_rows.begin(), new_rows.end());
        checkpoint(build);
    }
    void add_one(uint64_t id, const std::vector<double>& row, int build, const char* what = "add")
    {
        if (failed) return;
        op = std::string(what) + " id " + std::to_string(id) + " at n=" + std::to_string(n());
        if (ix->add(id, row.data(), dim) != OK) die(op.c_str());
        ids.push_back(id);
        rows.insert(rows.end(), row.begin(), row.end());
        checkpoint(build);
    }
    void add_random(uint64_t& rng, uint64_t id, int build)
    {
        std::vector<double> r(dim);
        random_row(rng, dim, r.data());
        add_one(id, r, build);
    }
    void remove_id(uint64_t id, int build, const char* what = "delete")
    {
        if (failed) return;
        std::string at;
        uint64_t first = ~0ull, w = 0;
        for (uint64_t p = 0; p < n(); ++p) {
            if (ids[p] == id) {
                if (first == ~0ull) first = p;
                at += (at.empty() ? "" : ",") + std::to_string(p);
                continue;
            }
            if (w != p) {
                ids[w] = ids[p];
                memcpy(&rows[w * dim], &rows[p * dim], dim * sizeof(double));
            }
            ++w;
        }
        op = std::string(what) + " id " + std::to_string(id) + " at position " + (at.empty() ? "none" : at) + " of n=" + std::to_string(n());
        ids.resize(w);
        rows.resize(w * dim);
        if (first != ~0ull) touched(first);
        if (ix->remove(id) != OK) die(op.c_str());
        checkpoint(build);
    }
    void remove_at(uint64_t pos, int build) { remove_id(ids[pos], build); }
    void truncate(uint64_t len, int build)
    {
        if (failed) return;
        op = "truncate to " + std::to_string(len) + " of n=" + std::to_string(n());
        if (len < n()) {
            ids.resize(len);
            rows.resize(len * dim);
            touched(len);
        }
        ix->truncate(len);
        checkpoint(build);
    }
    void refused_duplicate(uint64_t& rng, uint64_t id, int build)
    {
        if (failed) return;
        op = "refused duplicate add of id " + std::to_string(id);
        std::vector<double> r(dim);
        random_row(rng, dim, r.data());
        const uint64_t before = DerivedCopiesProbe(ix).mutations();
        if (ix->add(id, r.data(), dim) != ERR_DUP_ID) return fail("add", -1, -1, "a duplicate id was not refused with VL_ERR_DUP_ID");
        if (DerivedCopiesProbe(ix).mutations() != before) fail("mutations_", -1, -1, "moved by a refused add");
        checkpoint(build);
    }
    void refused_dimension(int build)
    {
        if (failed) return;
        op = "refused add of dimension " + std::to_string(dim + 1);
        const std::vector<double> r(dim + 1, 1.0);
        const uint64_t before = DerivedCopiesProbe(ix).mutations();
        if (ix->add(999999999999ull, r.data(), dim + 1) != ERR_DIM_MISMATCH)
            return fail("add", -1, -1, "a wrong dimension was not refused with VL_ERR_DIM_MISMATCH");
        if (DerivedCopiesProbe(ix).mutations() != before) fail("mutations_", -1, -1, "moved by a refused add");
        checkpoint(build);
    }
    void build_only(int build, const char* what)
    {
        if (failed) return;
        op = what;
        checkpoint(build);
    }
    // the clone takes over: a new handle with nothing derived beyond the ingest, the filters created again on it
    void clone_takes_over(int build)
    {
        if (failed) return;
        op = "clone at n=" + std::to_string(n());
        GpuFlatIndex* c = nullptr;
        if (ix->clone(&c) != OK) die("clone");
        delete ix;
        ix = c;
        for (uint64_t& b : bound) b = 0;
        shrunk = false;
        create_filters();
        checkpoint(build);
    }
};

struct Timer {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double s() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
};

void fill_rows(uint64_t& rng, uint32_t dim, uint64_t count, std::vector<double>* out)
{
    out->resize(count * dim);
    for (uint64_t i = 0; i < count; ++i) random_row(rng, dim, out->data() + i * dim);
}

// ---------------------------------------------------------------------------------------------
// a: watermarks and boundaries
// ---------------------------------------------------------------------------------------------
// deletes at the edges of the index, of a 16-row fragment group and of a 64-row MFMA tile, each right after a build of
// `before`; every delete is followed by a checkpoint that builds nothing and by one that builds `after`
void boundary_deletes(Audit& a, int before, int after)
{
    const auto at = [&](uint64_t pos) {
        a.build_only(before, "build before a boundary delete");
        a.remove_at(pos, 0);
        a.build_only(after, "rebuild after a boundary delete");
    };
    at(0);
    at(a.n() - 1);
    at(496);  // p % 16 == 0
    at(527);  // p % 16 == 15
    at(640);  // p % 64 == 0
    at(703);  // p % 64 == 63
    at(a.n() - 2);
}

bool stream_a(uint32_t dim)
{
    const Timer tm;
    Audit a(dim);
    uint64_t rng = 0xA0000 + dim;
    std::vector<uint64_t> ids(1000);
    std::vector<double> rows;
    for (uint64_t i = 0; i < 1000; ++i) ids[i] = 1 + i;
    fill_rows(rng, dim, 1000, &rows);
    a.op = "bulk add of 1000";
    if (a.ix->add_bulk(ids.data(), rows.data(), 1000, true, false) != OK) a.die("add_bulk");
    a.ids = ids;
    a.rows = rows;
    if (a.ix->capacity() != 1024) a.fail("capacity", (long long)a.ix->capacity(), 1024);
    {  // ids the index holds now, ids it will hold later (5000.. single adds, 20000.. the bulk add, 70000.. special rows), absent ids
        std::vector<uint64_t> fa, fb, gi, gk;
        for (uint64_t id = 1; id <= 1000; id += 3) fa.push_back(id);
        for (uint64_t id = 5000; id < 5100; id += 2) fa.push_back(id);
        for (uint64_t id = 20000; id < 21100; id += 5) fa.push_back(id);
        fa.push_back(123456789);
        for (uint64_t id = 1; id <= 1000; ++id)
            if (splitmix(rng) % 10 == 0) fb.push_back(id);
        for (uint64_t id : {1ull, 1000ull, 101ull, 70000ull, 70001ull, 70002ull, 5000ull, 5029ull, 987654321ull}) fb.push_back(id);
        for (uint64_t id = 20000; id < 21100; id += 3) fb.push_back(id);
        for (uint64_t id = 1; id <= 1000; ++id)
            if (id % 4 != 0) {
                gi.push_back(id);
                gk.push_back(1000 + id % 7);
            }
        for (uint64_t id = 5000; id < 5100; ++id) {
            gi.push_back(id);
            gk.push_back(1000 + id % 5);
        }
        for (uint64_t id = 20000; id < 21100; id += 2) {
            gi.push_back(id);
            gk.push_back(2000 + id % 11);
        }
        gi.push_back(70001);
        gk.push_back(3000);
        a.set_filters(fa, fb, gi, gk);
    }
    a.checkpoint(M_ALL);

    // single adds across 1024: the store grows at 1025 and frees the copies built just before
    const int schedule[8] = {0, M_ROW, M_FRAG | M_IDS, M_I8, M_ROW | M_I8, M_FRAG, M_ALL, M_IDS};
    uint64_t next = 5000;
    for (int i = 0; i < 30; ++i) a.add_random(rng, next++, a.n() + 1 == 1024 ? M_ALL : schedule[i % 8]);
    if (!a.failed && a.ix->capacity() != 2048) a.fail("capacity", (long long)a.ix->capacity(), 2048);

    boundary_deletes(a, M_ALL, M_ALL);
    boundary_deletes(a, M_FRAG, M_FRAG);  // the fragment copy alone is current; the others keep whatever they had
    boundary_deletes(a, M_ROW, M_ROW);    // the row-major copy alone
    boundary_deletes(a, M_I8 | M_IDS, M_FRAG | M_I8);

    // a bulk add across 2048: the store grows again
    {
        std::vector<uint64_t> bi(1100);
        std::vector<double> br;
        for (uint64_t i = 0; i < 1100; ++i) bi[i] = 20000 + i;
        fill_rows(rng, dim, 1100, &br);
        a.build_only(M_ALL, "build before the bulk add");
        a.add_bulk(bi, br, true, 0, "bulk add");
        if (!a.failed && a.ix->capacity() != 4096) a.fail("capacity", (long long)a.ix->capacity(), 4096);
        a.build_only(M_ROW | M_I8, "build after the bulk add");
        boundary_deletes(a, M_FRAG | M_IDS, M_ROW);
    }

    // an id stored at three positions, one of them the last (unvalidated rows), deleted in one call
    if (!a.failed) {
        uint64_t at = 100;  // a row both filters' neighbourhoods see: the first one from 100 on that filter A holds
        while (!std::binary_search(a.fset[0].begin(), a.fset[0].end(), a.ids[at])) ++at;
        const uint64_t dup = a.ids[at];
        std::vector<double> br;
        fill_rows(rng, dim, 3, &br);
        a.add_bulk({dup, 30000, dup}, br, false, M_ALL, "unvalidated bulk add");
        a.remove_id(dup, 0, "delete of a triple");
        a.build_only(M_ALL, "rebuild after the triple");
    }
    a.remove_id(424242424242ull, schedule[3], "delete of an absent");

    // truncate to a length that is no multiple of 16, then adds
    if (!a.failed) {
        uint64_t len = a.n() - 37;
        if (len % 16 == 0) --len;
        a.truncate(len, 0);
        a.build_only(M_FRAG, "build of the fragment copy after truncate");
        for (int i = 0; i < 5; ++i) a.add_random(rng, next++, schedule[(i + 1) % 8]);
        a.build_only(M_ALL, "build before the second truncate");
        a.truncate(a.n() - 21, M_ROW);
        for (int i = 0; i < 20; ++i) a.add_random(rng, next++, schedule[(i + 3) % 8]);
        a.truncate(a.n() + 5, M_ALL);  // not shorter: nothing happens
    }

    // rows outside the fast-path domain and a zero row, then their deletion
    if (!a.failed) {
        std::vector<double> r(dim);
        random_row(rng, dim, r.data());
        r[3] = 0x1.0p41;
        a.add_one(70000, r, M_I8, "add of an out-of-domain (2^41)");
        std::fill(r.begin(), r.end(), 0.0);
        r[0] = 0x1.0p-45;
        a.add_one(70001, r, M_FRAG, "add of a tiny (norm 2^-45)");
        r[0] = 0.0;
        a.add_one(70002, r, M_ALL, "add of a zero");
        a.add_random(rng, next++, 0);
        if (!a.failed && DerivedCopiesProbe(a.ix).n_out_of_domain() != 2) a.fail("n_out_of_domain_", (long long)DerivedCopiesProbe(a.ix).n_out_of_domain(), 2);
        a.remove_id(70000, 0);
        a.remove_id(70002, M_ROW | M_IDS);
        a.remove_id(70001, M_ALL);
    }

    a.refused_duplicate(rng, a.failed ? 0 : a.ids[7], 0);
    a.refused_dimension(M_ALL);
    printf("stream a dim=%u: %d checkpoints, n=%llu, %.2f s\n", dim, a.ckpt, (unsigned long long)a.n(), tm.s());
    return !a.failed;
}

// ---------------------------------------------------------------------------------------------
// b: a seeded random stream
// ---------------------------------------------------------------------------------------------
bool stream_b(uint64_t seed)
{
    const Timer tm;
    const uint32_t dim = 128;
    const uint64_t n0 = 3000;
    Audit a(dim);
    uint64_t rng = seed * 0x2545F4914F6CDD1Dull + 0xB;
    std::vector<uint64_t> ids(n0);
    std::vector<double> rows;
    for (uint64_t i = 0; i < n0; ++i) ids[i] = (i * 2654435761ull) % 1000003ull + 1;  // distinct, unordered
    fill_rows(rng, dim, n0, &rows);
    a.op = "bulk add of 3000";
    if (a.ix->add_bulk(ids.data(), rows.data(), n0, false, false) != OK) a.die("add_bulk");
    a.ids = ids;
    a.rows = rows;
    uint64_t next = 1000000000000ull;
    {
        std::vector<uint64_t> fa, fb, gi, gk;
        for (uint64_t id : ids) {
            if (splitmix(rng) % 2) fa.push_back(id);
            if (splitmix(rng) % 10 == 0) fb.push_back(id);
            if (splitmix(rng) % 3) {
                gi.push_back(id);
                gk.push_back(id % 13);
            }
        }
        for (uint64_t id = next; id < next + 6000; ++id) {  // ids the stream will add
            if (id % 2) fa.push_back(id);
            if (id % 7 == 0) fb.push_back(id);
            if (id % 3) {
                gi.push_back(id);
                gk.push_back(100 + id % 5);
            }
        }
        a.set_filters(fa, fb, gi, gk);
    }
    a.checkpoint(M_ALL);
    for (int step = 0; step < 150 && !a.failed; ++step) {
        const int build = (int)(splitmix(rng) & 15);
        switch (splitmix(rng) % 8) {
        case 0: a.add_random(rng, next++, build); break;
        case 1: {
            const uint64_t c = 1 + splitmix(rng) % 59;
            std::vector<uint64_t> bi(c);
            std::vector<double> br;
            for (uint64_t i = 0; i < c; ++i) bi[i] = next++;
            fill_rows(rng, dim, c, &br);
            a.add_bulk(bi, br, true, build, "bulk add");
            break;
        }
        case 2:
            if (a.n()) a.remove_at(splitmix(rng) % a.n(), build);
            break;
        case 3: a.remove_id(7, build, "delete of an absent"); break;
        case 4:
            if (a.n()) a.refused_duplicate(rng, a.ids[0], build);
            break;
        case 5: a.refused_dimension(build); break;
        case 6: a.clone_takes_over(build); break;
        default:
            if (a.n() > 50) a.truncate(a.n() - 1 - splitmix(rng) % 40, build);
            break;
        }
    }
    printf("stream b seed=%llu: %d checkpoints, n=%llu, %.2f s\n", (unsigned long long)seed, a.ckpt, (unsigned long long)a.n(), tm.s());
    return !a.failed;
}

// ---------------------------------------------------------------------------------------------
// c: the delete's bounce loop
// ---------------------------------------------------------------------------------------------
bool stream_c()
{
    const Timer tm;
    const uint32_t dim = 1000;  // 8000-byte master rows: a 64 MB chunk ends inside a row
    const uint64_t n0 = 9000;   // 72 MB of master rows: deleting row 0 moves them in two chunks
    Audit a(dim);
    uint64_t rng = 0xC;
    std::vector<uint64_t> ids(n0);
    std::vector<double> rows;
    for (uint64_t i = 0; i < n0; ++i) ids[i] = 1 + i;
    fill_rows(rng, dim, n0, &rows);
    a.op = "bulk add of 9000";
    if (a.ix->add_bulk(ids.data(), rows.data(), n0, true, false) != OK) a.die("add_bulk");
    a.ids = ids;
    a.rows = rows;
    {
        std::vector<uint64_t> fa, fb, gi, gk;
        for (uint64_t id = 1; id <= n0; ++id) {
            if (id % 2) fa.push_back(id);
            if (id % 97 == 1) fb.push_back(id);
            if (id % 5) {
                gi.push_back(id);
                gk.push_back(id % 31);
            }
        }
        a.set_filters(fa, fb, gi, gk);
    }
    a.checkpoint(M_ALL);
    a.remove_at(0, 0);
    a.build_only(M_ALL, "rebuild after the delete at 0");
    a.remove_at(500, M_ROW | M_I8);
    printf("stream c: %d checkpoints, n=%llu, %.2f s\n", a.ckpt, (unsigned long long)a.n(), tm.s());
    return !a.failed;
}

}  // namespace

int main(int argc, char** argv)
{
    setvbuf(stdout, nullptr, _IOLBF, 0);
    bool ok;
    if (argc == 2 && strcmp(argv[1], "a") == 0) {
        ok = stream_a(100);
        ok = ok && stream_a(384);
    } else if ((argc == 2 || argc == 3) && strcmp(argv[1], "b") == 0) {
        ok = stream_b(argc == 3 ? strtoull(argv[2], nullptr, 10) : 1);
    } else if (argc == 2 && strcmp(argv[1], "c") == 0) {
        ok = stream_c();
    } else {
        printf("usage: derived_copies_audit a | b [seed] | c\n");
        return 2;
    }
    printf(ok ? "audit ok\n" : "audit FAILED\n");
    return ok ? 0 : 1;
}
