// Audit of every device copy a flat index derives from its f64 master rows, after in-place updates and upserts
// (GpuFlatIndex::update / update_bulk; test tool, not shipped; driven by
// tests/test_gpu_update_copies_audit.py).  The sibling of derived_copies_audit.hip, which audits add / delete / truncate.
//
//   update_copies_audit a          boundaries and watermarks: a scripted stream at dim 100 and dim 384, 2100 rows
//   update_copies_audit b [seed]   a seeded random stream at dim 128 (3000 rows, 150 operations)
//
// The program keeps a plain host mirror of the index (ids and f64 rows; an update overwrites the first row with the id, an
// upsert is the sequential loop of the contract) and, after every operation, takes a CHECKPOINT: the mirror's rows are
// uploaded to a scratch master and converted from row 0 by the library's own launchers (launch_ingest, launch_rows_bf16,
// launch_rows_i8); the index's state must equal that from-scratch state.  Bytes and integers only:
//   - len(), the exported ids and master bits;
//   - the f32 slab (padding included), inv_norm, the device flags, row_flags_, n_out_of_domain_; max_row_norm_ is an upper
//     bound (it may stay high after an update or a delete) and exact while neither happened;
//   - the lazy copies below the watermark the index goes by: the row-major and the fragment-major bf16 copy with norm16 /
//     sqnorm, the int8 copy with its (s, r) pairs and |row|;
//   - the watermarks: a copy built at this checkpoint stands at n; an update moves none of them (read before and after the
//     call), whatever it rewrote; mutations_ moves by exactly one when an upsert appended rows and not at all otherwise.
// One line per failed comparison, then "audit ok" or "audit FAILED" (exit status 1).  The stream stops at the first failing
// checkpoint.
#include "../../vectorlite_amd/csrc/flat_index.hpp"
#include "../../vectorlite_amd/csrc/update_plan.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
    uint64_t watermark(int copy) const
    {
        const uint64_t w[3] = {ix->slab16_rows_, ix->slab16f_rows_, ix->slab8_rows_};
        return w[copy];
    }
    const std::vector<uint8_t>& row_flags() const { return ix->row_flags_; }
    uint64_t n_out_of_domain() const { return ix->n_out_of_domain_; }
    double max_row_norm() const { return ix->max_row_norm_; }
    uint64_t mutations() const { return ix->mutations_; }
    // the lazy builds, called as the search routes call them: under the shared index lock
    int ensure(int copy) const
    {
        std::shared_lock<RwLock> lk(ix->mu_);
        if (hipSetDevice(ix->device_) != hipSuccess) return ERR_DEVICE;
        switch (copy) {
        case 0: return ix->ensure_bf16_slab(false);
        case 1: return ix->ensure_bf16_slab(true);
        default: return ix->ensure_i8_slab();
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

enum Copy : int { C_ROW = 0, C_FRAG = 1, C_I8 = 2 };
constexpr int M_ROW = 1, M_FRAG = 2, M_I8 = 4, M_ALL = 7;
const char* const COPY_NAME[3] = {"slab16_rows_", "slab16f_rows_", "slab8_rows_"};

uint64_t splitmix(uint64_t& x)
{
    uint64_t z = (x += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
double uniform01(uint64_t& x) { return ((double)(splitmix(x) >> 11) + 0.5) * 0x1.0p-53; }
double normal(uint64_t& x) { return std::sqrt(-2.0 * std::log(uniform01(x))) * std::cos(6.283185307179586 * uniform01(x)); }

// a gaussian direction at norm 0.25, 1 or 4 times a per-row factor in [1, 1 + 2^-4): every row differs from every other in
// every per-row array, so a row left stale or written to a neighbour's place differs in its bytes
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

struct Fresh {  // the from-scratch state of n rows
    std::vector<float> slab, inv, n16, sq, sr8, n8;
    std::vector<uint8_t> flags, b8;
    std::vector<uint16_t> b16;
    double max_norm = 0.0;
};

struct Audit {
    uint32_t dim, ld, ldb;
    bool frag_ok;
    GpuFlatIndex* ix = nullptr;
    std::vector<uint64_t> ids;  // the mirror
    std::vector<double> rows;
    bool loose_norm = false;  // an update or a delete happened: max_row_norm_ may stay high
    bool failed = false;
    int ckpt = 0;
    uint64_t updates = 0, rewritten[3] = {0, 0, 0};
    std::string op = "start";
    hipStream_t stream = nullptr;
    DevBuf<double> s_master;
    DevBuf<float> s_slab, s_inv, s_n16, s_sq, s_sr8, s_n8;
    DevBuf<uint8_t> s_flags, s_b8;
    DevBuf<uint16_t> s_b16;
    DevBuf<IngestStats> s_stats;

    Audit(uint32_t d, uint64_t reserve_rows) : dim(d), ld((d + 3u) & ~3u), ldb(mfma_ldb(d))
    {
        frag_ok = mfma_rows_kernel(d) && ldb % 32 == 0;
        CK(hipStreamCreate(&stream));
        if (GpuFlatIndex::create(d, 0, &ix) != OK || ix->reserve(reserve_rows) != OK) die("create");
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
        const IngestStats st = download(s_stats.p, 1)[0];
        memcpy(&f.max_norm, &st.max_norm_bits, 8);
        return f;
    }

    void check_copy(const DerivedCopiesProbe& pr, const Fresh& f, int c, uint64_t w)
    {
        if (w == 0) return;
        if (c == C_ROW) {
            if (!pr.slab16() || !pr.norm16()) return fail("d_slab16_", -1, -1, "null with a watermark above 0");
            same("d_slab16_", download(static_cast<const uint16_t*>(pr.slab16()), w * ldb).data(), f.b16.data(), w, ldb, 2);
        } else if (c == C_FRAG) {
            if (!pr.slab16f() || !pr.norm16()) return fail("d_slab16f_", -1, -1, "null with a watermark above 0");
            const uint64_t groups = (w + 15) / 16;
            const uint32_t ks32 = ldb / 32;
            const std::vector<unsigned char> fr = download(static_cast<const unsigned char*>(pr.slab16f()), groups * 16 * ldb * 2);
            for (uint64_t r = 0; r < w; ++r)
                for (uint32_t p = 0; p < ldb / 8; ++p) {
                    const size_t off = ((((size_t)(r >> 4) * ks32 + (p >> 2)) * 64) + (size_t)((p & 3) * 16 + (uint32_t)(r & 15))) * 16;
                    if (memcmp(&fr[off], &f.b16[r * ldb + 8 * p], 16) != 0) return fail("d_slab16f_", (long long)r, (long long)(8 * p));
                }
        } else {
            if (!pr.slab8() || !pr.sr8() || !pr.norm8()) return fail("d_slab8_", -1, -1, "null with a watermark above 0");
            same("d_slab8_", download(static_cast<const uint8_t*>(pr.slab8()), w * ldb).data(), f.b8.data(), w, ldb, 1);
            same("d_sr8_", download(pr.sr8(), 2 * w).data(), f.sr8.data(), w, 2, 4);
            same("d_norm8_", download(pr.norm8(), w).data(), f.n8.data(), w, 1, 4);
        }
    }

    // `build` names the lazy copies built now
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
        if (!(pr.max_row_norm() >= f.max_norm) || (!loose_norm && pr.max_row_norm() != f.max_norm)) {
            char note[96];
            snprintf(note, sizeof note, "held %.17g fresh %.17g", pr.max_row_norm(), f.max_norm);
            fail("max_row_norm_", -1, -1, note);
        }
        if (failed) return;
        for (int c = 0; c < 3; ++c)
            if (build & (1 << c)) {
                if (pr.ensure(c) != OK) die("ensure");
                if (pr.watermark(c) != m) fail(COPY_NAME[c], (long long)pr.watermark(c), (long long)m, "(row = watermark after its build, col = n)");
            } else if (pr.watermark(c) > m) {
                fail(COPY_NAME[c], (long long)pr.watermark(c), (long long)m, "(row = watermark, col = n)");
            }
        for (int c = 0; c < 3; ++c) check_copy(pr, f, c, std::min<uint64_t>(pr.watermark(c), m));
        const uint64_t wn = std::min<uint64_t>(std::max(pr.watermark(C_ROW), pr.watermark(C_FRAG)), m);  // shared by both bf16 copies
        if (wn && pr.norm16() && pr.sqnorm()) {
            same("d_norm16_", download(pr.norm16(), wn).data(), f.n16.data(), wn, 1, 4);
            same("d_sqnorm_", download(pr.sqnorm(), wn).data(), f.sq.data(), wn, 1, 4);
        }
    }

    // ---- operations, applied to the index and to the mirror ----
    uint64_t find(uint64_t id) const { return (uint64_t)(std::find(ids.begin(), ids.end(), id) - ids.begin()); }

    // update_bulk / upsert: the mirror runs the contract's loop; the call must report its counts, move mutations_ by one
    // iff it appended, and leave every watermark where it was (the store was reserved: nothing grows)
    void update_many(const std::vector<uint64_t>& lst, const std::vector<double>& vals, bool insert_missing, int build, const char* what)
    {
        if (failed) return;
        op = std::string(what) + " of " + std::to_string(lst.size()) + " at n=" + std::to_string(n());
        const uint64_t n_before = n();
        std::vector<uint8_t> hit(n_before, 0);
        for (size_t i = 0; i < lst.size(); ++i) {
            const uint64_t p = find(lst[i]);
            if (p < n()) {
                memcpy(&rows[p * dim], &vals[i * dim], dim * sizeof(double));
                if (p < n_before) hit[p] = 1;
            } else {
                if (!insert_missing) die("the audit's own list names an absent id");
                ids.push_back(lst[i]);
                rows.insert(rows.end(), vals.begin() + i * dim, vals.begin() + (i + 1) * dim);
            }
        }
        const uint64_t want_upd = (uint64_t)std::count(hit.begin(), hit.end(), 1), want_ins = n() - n_before;
        const DerivedCopiesProbe pr(ix);
        const uint64_t mut0 = pr.mutations(), w0[3] = {pr.watermark(0), pr.watermark(1), pr.watermark(2)}, cap0 = ix->capacity();
        uint64_t upd = ~0ull, ins = ~0ull;
        if (ix->update_bulk(lst.data(), vals.data(), lst.size(), insert_missing, &upd, &ins) != OK) die(op.c_str());
        if (upd != want_upd || ins != want_ins) fail("update_bulk counts", (long long)upd, (long long)ins, "(row = updated, col = inserted)");
        if (pr.mutations() != mut0 + (want_ins ? 1 : 0)) fail("mutations_", (long long)pr.mutations(), (long long)mut0, "(row = after, col = before)");
        if (ix->capacity() != cap0) fail("capacity", (long long)ix->capacity(), (long long)cap0, "the reserved store grew");
        uint64_t st[7];
        ix->last_update(st);
        if (st[0] != want_upd || st[1] != want_ins) fail("last_update", (long long)st[0], (long long)st[1]);
        for (int c = 0; c < 3; ++c) {
            if (pr.watermark(c) != w0[c]) fail(COPY_NAME[c], (long long)pr.watermark(c), (long long)w0[c], "(row = after the update, col = before)");
            uint64_t below = 0;
            for (uint64_t p = 0; p < n_before; ++p) below += hit[p] && p < w0[c];
            if (st[2 + c] != below) fail("last_update rows per copy", (long long)st[2 + c], (long long)below, COPY_NAME[c]);
            rewritten[c] += below;
        }
        ++updates;
        loose_norm = true;
        checkpoint(build);
    }
    void update_at(const std::vector<uint64_t>& positions, uint64_t& rng, int build, const char* what)
    {
        if (failed) return;
        std::vector<uint64_t> lst;
        std::vector<double> vals(positions.size() * dim);
        for (size_t i = 0; i < positions.size(); ++i) {
            lst.push_back(ids[positions[i]]);
            random_row(rng, dim, &vals[i * dim]);
        }
        update_many(lst, vals, false, build, what);
    }
    void update_one(uint64_t pos, const std::vector<double>& row, int build, const char* what)
    {
        if (failed) return;
        op = std::string(what) + " at position " + std::to_string(pos);
        const uint64_t id = ids[pos], first = find(id);
        memcpy(&rows[first * dim], row.data(), dim * sizeof(double));
        const DerivedCopiesProbe pr(ix);
        const uint64_t mut0 = pr.mutations(), w0[3] = {pr.watermark(0), pr.watermark(1), pr.watermark(2)};
        if (ix->update(id, row.data(), dim) != OK) die(op.c_str());
        if (pr.mutations() != mut0) fail("mutations_", (long long)pr.mutations(), (long long)mut0, "moved by a pure update");
        for (int c = 0; c < 3; ++c)
            if (pr.watermark(c) != w0[c]) fail(COPY_NAME[c], (long long)pr.watermark(c), (long long)w0[c], "(row = after the update, col = before)");
        ++updates;
        loose_norm = true;
        checkpoint(build);
    }
    void refused(const std::vector<uint64_t>& lst, uint64_t len, int want_rc, int build, const char* what)
    {
        if (failed) return;
        op = what;
        const std::vector<double> vals(lst.size() * (size_t)len, 0.5);
        const DerivedCopiesProbe pr(ix);
        const uint64_t mut0 = pr.mutations();
        uint64_t upd = 7, ins = 7;
        const int rc = lst.size() == 1 && len != dim ? ix->update(lst[0], vals.data(), len)
                                                      : ix->update_bulk(lst.data(), vals.data(), lst.size(), false, &upd, &ins);
        if (rc != want_rc) return fail("refusal", rc, want_rc, "(row = status, col = expected)");
        if (pr.mutations() != mut0) fail("mutations_", -1, -1, "moved by a refused update");
        uint64_t st[7];
        ix->last_update(st);
        for (uint64_t v : st)
            if (v) fail("last_update", (long long)v, 0, "not all zero after a refused call");
        checkpoint(build);
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
    void remove_ids(const std::vector<uint64_t>& gone, bool bulk, int build, const char* what)
    {
        if (failed) return;
        op = std::string(what) + " of " + std::to_string(gone.size()) + " at n=" + std::to_string(n());
        uint64_t w = 0;
        for (uint64_t p = 0; p < n(); ++p) {
            if (std::find(gone.begin(), gone.end(), ids[p]) != gone.end()) continue;
            if (w != p) {
                ids[w] = ids[p];
                memcpy(&rows[w * dim], &rows[p * dim], dim * sizeof(double));
            }
            ++w;
        }
        ids.resize(w);
        rows.resize(w * dim);
        loose_norm = true;
        if (bulk) {
            if (ix->remove_bulk(gone.data(), gone.size(), nullptr, nullptr) != OK) die(op.c_str());
        } else {
            for (uint64_t id : gone)
                if (ix->remove(id) != OK) die(op.c_str());
        }
        checkpoint(build);
    }
    void build_only(int build, const char* what)
    {
        if (failed) return;
        op = what;
        checkpoint(build);
    }
    // the clone takes over: a new handle with nothing derived beyond the ingest; the original goes
    void clone_takes_over(uint64_t reserve_rows, int build)
    {
        if (failed) return;
        op = "clone at n=" + std::to_string(n());
        GpuFlatIndex* c = nullptr;
        if (ix->clone(&c) != OK || c->reserve(reserve_rows) != OK) die("clone");
        delete ix;
        ix = c;
        loose_norm = false;
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
// a: boundaries and watermarks
// ---------------------------------------------------------------------------------------------
bool stream_a(uint32_t dim)
{
    const Timer tm;
    const uint64_t n0 = 2100, reserve = 4096;  // 2100 = 131 whole 16-row groups and a partial one of 4
    Audit a(dim, reserve);
    uint64_t rng = 0xD0000 + dim;
    std::vector<uint64_t> ids(n0);
    std::vector<double> rows;
    for (uint64_t i = 0; i < n0; ++i) ids[i] = 1 + i;
    fill_rows(rng, dim, n0, &rows);
    a.add_bulk(ids, rows, true, 0, "bulk add");
    // positions 0, 15, 16, 31, 32, 63, 64, the last row of the last whole 16-row group, the first and the last row of the
    // partial group (the last row of the index)
    const std::vector<uint64_t> edges = {0, 15, 16, 31, 32, 63, 64, 2095, 2096, 2099};

    // no lazy copy built; then each one alone (a clone has none)
    a.update_at(edges, rng, 0, "update of the boundary rows, no lazy copy");
    for (uint64_t p : {0ull, 15ull, 2099ull}) {
        std::vector<double> r(dim);
        random_row(rng, dim, r.data());
        a.update_one(p, r, 0, "single update, no lazy copy");
    }
    for (int alone : {M_ROW, M_FRAG, M_I8}) {
        a.clone_takes_over(reserve, alone);
        a.update_at(edges, rng, 0, "update of the boundary rows, one lazy copy");
        for (uint64_t p : {16ull, 63ull, 2096ull}) {
            std::vector<double> r(dim);
            random_row(rng, dim, r.data());
            a.update_one(p, r, 0, "single update, one lazy copy");
        }
        a.build_only(M_ALL, "build of every copy after the updates");
        a.update_at(edges, rng, 0, "update of the boundary rows, every lazy copy");
    }

    // watermarks apart: row-major and int8 at 2100, fragment-major at 2150, n = 2180
    a.clone_takes_over(reserve, M_ROW | M_I8);
    {
        std::vector<uint64_t> bi(50);
        std::vector<double> br;
        for (uint64_t i = 0; i < 50; ++i) bi[i] = 20000 + i;
        fill_rows(rng, dim, 50, &br);
        a.add_bulk(bi, br, true, M_FRAG, "bulk add, then a build of the fragment-major copy alone");
        bi.resize(30);
        for (uint64_t i = 0; i < 30; ++i) bi[i] = 30000 + i;
        fill_rows(rng, dim, 30, &br);
        a.add_bulk(bi, br, true, 0, "bulk add without a build");
        if (!a.failed) {
            const DerivedCopiesProbe pr(a.ix);
            const uint64_t want[3] = {2100, a.frag_ok ? 2150u : 0u, 2100};
            for (int c = 0; c < 3; ++c)
                if (pr.watermark(c) != want[c]) a.fail(COPY_NAME[c], (long long)pr.watermark(c), (long long)want[c], "the script's watermarks");
        }
        // below, at and above each watermark, in one call and one by one
        const std::vector<uint64_t> around = {2099, 2100, 2101, 2149, 2150, 2151, 2179, 2096, 2111, 2112};
        a.update_at(around, rng, 0, "update around the watermarks");
        for (uint64_t p : around) {
            std::vector<double> r(dim);
            random_row(rng, dim, r.data());
            a.update_one(p, r, 0, "single update around the watermarks");
        }
        a.build_only(M_ALL, "conversion of the rows above the watermarks from the updated master");
        a.update_at(around, rng, M_ALL, "update with every watermark at n");
    }

    // in the domain -> out of it -> back; a zero row; a tiny row
    if (!a.failed) {
        std::vector<double> r(dim), keep(a.rows.begin() + 16 * dim, a.rows.begin() + 17 * dim);
        random_row(rng, dim, r.data());
        r[3] = 0x1.0p41;
        a.update_one(16, r, 0, "update to an out-of-domain row (2^41)");
        if (!a.failed && DerivedCopiesProbe(a.ix).n_out_of_domain() != 1) a.fail("n_out_of_domain_", (long long)DerivedCopiesProbe(a.ix).n_out_of_domain(), 1);
        a.update_one(16, r, M_I8, "the same out-of-domain row again");
        if (!a.failed && DerivedCopiesProbe(a.ix).n_out_of_domain() != 1) a.fail("n_out_of_domain_", (long long)DerivedCopiesProbe(a.ix).n_out_of_domain(), 1);
        a.update_one(16, keep, M_ALL, "update back into the domain");
        if (!a.failed && DerivedCopiesProbe(a.ix).n_out_of_domain() != 0) a.fail("n_out_of_domain_", (long long)DerivedCopiesProbe(a.ix).n_out_of_domain(), 0);
        std::fill(r.begin(), r.end(), 0.0);
        a.update_one(31, r, 0, "update to a zero row");
        r[0] = 0x1.0p-45;
        a.update_one(2099, r, M_ALL, "update to a tiny row (norm 2^-45)");
        a.update_at({31, 2099}, rng, M_ALL, "update of the zero and the tiny row to gaussian rows");
    }

    // an id stored at three positions: only the first is rewritten
    if (!a.failed) {
        const uint64_t dup = a.ids[5];
        std::vector<double> br;
        fill_rows(rng, dim, 3, &br);
        a.add_bulk({dup, 40000, dup}, br, false, M_ALL, "unvalidated bulk add of a triple id");
        std::vector<double> r(dim);
        random_row(rng, dim, r.data());
        a.update_one(a.n() - 1, r, 0, "update of an id stored three times");  // names the id by its last row: the first one changes
        a.update_many({dup, 40000, dup}, br, false, M_ALL, "bulk update naming the triple id twice");
    }

    // refused calls: nothing changes
    a.refused({a.failed ? 0 : a.ids[3], 424242424242ull, a.failed ? 0 : a.ids[4]}, dim, ERR_NOT_FOUND, 0, "refused: an absent id among present ones");
    a.refused({a.failed ? 0 : a.ids[3]}, dim + 1, ERR_DIM_MISMATCH, M_ALL, "refused: a row of dim + 1 values");

    // a staging buffer of two rows: a 40-row update in 20 chunks; then an upsert through it
    if (!a.failed) {
        if (a.ix->set_delete_bounce(48 + 2 * ((uint64_t)dim * 8 + 5) + 1) != OK) a.die("set_delete_bounce");
        std::vector<uint64_t> pos;
        for (uint64_t i = 0; i < 40; ++i) pos.push_back((i * 53 + 7) % a.n());
        a.update_at(pos, rng, 0, "40-row update through a two-row staging buffer");
        uint64_t st[7];
        a.ix->last_update(st);
        if (!a.failed && st[5] != 20) a.fail("last_update chunks", (long long)st[5], 20);
        std::vector<uint64_t> lst = {a.ids[0], 50000, a.ids[2099], 50001, 50000, a.ids[64], 50002, a.ids[0]};
        std::vector<double> vals;
        fill_rows(rng, dim, lst.size(), &vals);
        a.update_many(lst, vals, true, M_ALL, "upsert through a two-row staging buffer");
    }
    printf("stream a dim=%u: %d checkpoints, %llu updates, rows rewritten per copy %llu / %llu / %llu, n=%llu, %.2f s\n", dim, a.ckpt,
           (unsigned long long)a.updates, (unsigned long long)a.rewritten[0], (unsigned long long)a.rewritten[1],
           (unsigned long long)a.rewritten[2], (unsigned long long)a.n(), tm.s());
    return !a.failed;
}

// ---------------------------------------------------------------------------------------------
// b: a seeded random stream
// ---------------------------------------------------------------------------------------------
bool stream_b(uint64_t seed)
{
    const Timer tm;
    const uint32_t dim = 128;
    const uint64_t n0 = 3000, reserve = 16384;
    Audit a(dim, reserve);
    uint64_t rng = seed * 0x2545F4914F6CDD1Dull + 0xB;
    std::vector<uint64_t> ids(n0);
    std::vector<double> rows;
    for (uint64_t i = 0; i < n0; ++i) ids[i] = (i * 2654435761ull) % 1000003ull + 1;  // distinct, unordered
    fill_rows(rng, dim, n0, &rows);
    a.add_bulk(ids, rows, false, M_ALL, "bulk add");
    uint64_t next = 1000000000000ull;
    for (int step = 0; step < 150 && !a.failed; ++step) {
        const int build = (int)(splitmix(rng) & 7);  // the copies this step's searches would build
        switch (splitmix(rng) % 9) {
        case 0:
        case 1: {  // single update
            std::vector<double> r(dim);
            random_row(rng, dim, r.data());
            a.update_one(splitmix(rng) % a.n(), r, build, "single update");
            break;
        }
        case 2:
        case 3: {  // bulk update with repeats
            const uint64_t c = 1 + splitmix(rng) % 80;
            std::vector<uint64_t> pos(c);
            for (uint64_t& p : pos) p = splitmix(rng) % a.n();
            if (c > 3) pos[c - 1] = pos[0];
            a.update_at(pos, rng, build, "bulk update");
            break;
        }
        case 4: {  // upsert: present, absent and repeated ids
            const uint64_t c = 1 + splitmix(rng) % 60;
            std::vector<uint64_t> lst(c);
            for (uint64_t i = 0; i < c; ++i) lst[i] = splitmix(rng) % 3 == 0 ? next + splitmix(rng) % 20 : a.ids[splitmix(rng) % a.n()];
            next += 20;
            std::vector<double> vals;
            fill_rows(rng, dim, c, &vals);
            a.update_many(lst, vals, true, build, "upsert");
            break;
        }
        case 5: {  // add
            const uint64_t c = 1 + splitmix(rng) % 59;
            std::vector<uint64_t> bi(c);
            std::vector<double> br;
            for (uint64_t i = 0; i < c; ++i) bi[i] = next++;
            fill_rows(rng, dim, c, &br);
            a.add_bulk(bi, br, true, build, "bulk add");
            break;
        }
        case 6: a.remove_ids({a.ids[splitmix(rng) % a.n()]}, false, build, "delete"); break;
        case 7: {  // delete_many
            std::vector<uint64_t> gone;
            for (int i = 0; i < 12; ++i) gone.push_back(a.ids[splitmix(rng) % a.n()]);
            gone.push_back(7);
            a.remove_ids(gone, true, build, "delete_many");
            break;
        }
        default: a.clone_takes_over(reserve, build); break;
        }
    }
    printf("stream b seed=%llu: %d checkpoints, %llu updates, rows rewritten per copy %llu / %llu / %llu, n=%llu, %.2f s\n",
           (unsigned long long)seed, a.ckpt, (unsigned long long)a.updates, (unsigned long long)a.rewritten[0],
           (unsigned long long)a.rewritten[1], (unsigned long long)a.rewritten[2], (unsigned long long)a.n(), tm.s());
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
    } else {
        printf("usage: update_copies_audit a | b [seed]\n");
        return 2;
    }
    printf(ok ? "audit ok\n" : "audit FAILED\n");
    return ok ? 0 : 1;
}
