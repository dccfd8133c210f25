// extern "C" surface of libmatchy_amd.so — see include/matchy_amd.h for the per-function reference citations.
#include "../../include/matchy_amd.h"

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <list>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "capi_internal.h"
#include "db_builder.h"
#include "db_image.h"
#include "engine.h"
#include "gz_stream.h"
#include "host_lookup.h"
#include "inflate_core.h"
#include "ndjson_host.h"
#include "netaddr.h"
#include "render_core.h"

using namespace mxy;
using namespace mxy::capi;

namespace {
thread_local std::string g_last_error;
}
void mxy::capi::set_error(const std::string& e) { g_last_error = e; }

namespace {

struct Builder {
    DatabaseBuilder b;
};

struct Db {
    std::shared_ptr<DbImage> img;
    std::mutex mu;                                   // guards dev + query scanner (single queries are serialised)
    std::vector<std::shared_ptr<DeviceDb>> dev;      // per device ordinal, uploaded on first use
    std::unique_ptr<Scanner> query_scanner;        // single queries through the lookup kernels (MATCHY_AMD_QUERY_ON_GPU=1: tests)
    std::unique_ptr<HostTables> host_tables;       // single queries on the host (host_lookup.h): built by the first query
    DevBuf<uint8_t> qbuf;
    DevBuf<Candidate> qcand;
    std::string format;
    int default_device = 0;
    // DatabaseStats (database.rs:728-795)
    mutable std::atomic<uint64_t> st_total{0}, st_match{0}, st_nomatch{0}, st_ip{0}, st_str{0}, st_chit{0}, st_cmiss{0};
    // Query cache of Database::lookup (database.rs:32-40, 384-407, 725-804): LRU keyed by the query string, holds "not found" too.
    // ONE PER THREAD AND HANDLE, like the reference's thread-local caches (round 5; until then one per handle behind `mu`, which made
    // eight querying threads slower than one): a query takes no lock. 0 entries = disabled (matchy_open_options_t.cache_capacity).
    struct Cached { int kind; uint8_t prefix_len; bool has_data; DataValue data; };   // kind: 0 not found, 2 IP, 3 pattern
    struct Lru {
        std::list<std::pair<std::string, Cached>> lru;
        std::unordered_map<std::string, std::list<std::pair<std::string, Cached>>::iterator> index;
        const Cached* get(const std::string& q) {
            auto it = index.find(q);
            if (it == index.end()) return nullptr;
            lru.splice(lru.begin(), lru, it->second);
            return &it->second->second;
        }
        void put(const std::string& q, Cached&& c, size_t cap) {
            if (!cap) return;
            auto it = index.find(q);
            if (it != index.end()) { it->second->second = std::move(c); lru.splice(lru.begin(), lru, it->second); return; }
            lru.emplace_front(q, std::move(c));
            index[q] = lru.begin();
            if (lru.size() > cap) { index.erase(lru.back().first); lru.pop_back(); }
        }
        void clear() { lru.clear(); index.clear(); }
    };
    size_t cache_cap = 10000;
    const uint64_t uid = next_uid();   // names this handle in the threads' cache maps (a pointer could be reused by a later handle)
    static uint64_t next_uid() { static std::atomic<uint64_t> n{1}; return n.fetch_add(1); }
    static std::mutex& live_mu() { static std::mutex m; return m; }
    static std::unordered_set<uint64_t>& live() { static std::unordered_set<uint64_t> s; return s; }
    Db() { std::lock_guard<std::mutex> lk(live_mu()); live().insert(uid); }
    ~Db() { std::lock_guard<std::mutex> lk(live_mu()); live().erase(uid); }
    // the calling thread's cache of this handle; caches of closed handles are dropped when a thread meets a new handle
    Lru& cache() {
        thread_local std::unordered_map<uint64_t, Lru> mine;
        auto it = mine.find(uid);
        if (it != mine.end()) return it->second;
        if (mine.size() >= 4) {
            std::lock_guard<std::mutex> lk(live_mu());
            for (auto k = mine.begin(); k != mine.end();) k = live().count(k->first) ? std::next(k) : mine.erase(k);
        }
        return mine[uid];
    }
    std::once_flag host_tables_once;

    std::shared_ptr<DeviceDb> device_db(int device) {
        if ((int)dev.size() <= device) dev.resize(device + 1);
        if (!dev[device]) {
            auto d = std::make_shared<DeviceDb>();
            d->upload(*img, device);
            dev[device] = d;
        }
        return dev[device];
    }
};

struct ExtractorH {
    std::shared_ptr<DbImage> img;  // empty image: only the PSL tables are needed
    std::shared_ptr<DeviceDb> ddb;
    std::unique_ptr<Scanner> scanner;
    std::mutex mu;
    uint32_t flags;
};

struct MatchesInternal {
    std::vector<matchy_match_t> items;
    std::vector<std::string> values;
};

struct ScannerH {
    const Db* db;
    std::unique_ptr<Scanner> sc;
    ndjson::Renderer ndjson;   // matchy_scan_result_to_ndjson*: the payload texts and the escaped source live across calls
    // matchy_scanner_submit_device -> matchy_scanner_wait
    bool pending = false;
    size_t pending_len = 0;
    uint32_t pending_mode = 0;
    void* pending_stream = nullptr;
    bool pending_hit_lines = false;   // the scanner's hit-lines setting when the batch was submitted
};

int type_rank(uint32_t t) {  // chunk-path extractor order (matchy-extractor/src/lib.rs:449-485)
    switch (t) {
        case IT_IPV6: return 0; case IT_IPV4: return 1; case IT_EMAIL: return 2; case IT_DOMAIN: return 3;
        case IT_MD5: case IT_SHA1: case IT_SHA256: case IT_SHA384: case IT_SHA512: return 4;
        case IT_BITCOIN: return 5; case IT_ETHEREUM: return 6; case IT_MONERO: return 7;
    }
    return 8;
}

bool valid_utf8_host(const uint8_t* s, size_t n) {
    size_t i = 0;
    while (i < n) {
        uint8_t c = s[i];
        if (c < 0x80) { ++i; continue; }
        size_t l = (c >= 0xC2 && c <= 0xDF) ? 2 : (c >= 0xE0 && c <= 0xEF) ? 3 : (c >= 0xF0 && c <= 0xF4) ? 4 : 0;
        if (l == 0 || i + l > n) return false;
        uint8_t lo = 0x80, hi = 0xBF;
        if (c == 0xE0) lo = 0xA0;
        if (c == 0xED) hi = 0x9F;
        if (c == 0xF0) lo = 0x90;
        if (c == 0xF4) hi = 0x8F;
        if (s[i + 1] < lo || s[i + 1] > hi) return false;
        for (size_t k = 2; k < l; ++k) if ((s[i + k] & 0xC0) != 0x80) return false;
        i += l;
    }
    return true;
}

const char* item_type_name(uint8_t t) {
    static const char* N[] = {"Domain", "Email", "IPv4", "IPv6", "MD5", "SHA1", "SHA256", "SHA384", "SHA512", "Bitcoin", "Ethereum", "Monero"};
    return t < 12 ? N[t] : "Unknown";
}

bool read_file(const char* path, std::vector<uint8_t>& out) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    uint8_t tmp[1 << 16];
    size_t n;
    while ((n = fread(tmp, 1, sizeof(tmp), f)) > 0) out.insert(out.end(), tmp, tmp + n);
    fclose(f);
    return true;
}

matchy_t* open_bytes(std::vector<uint8_t>&& bytes) {
    try {
        const bool trace = getenv("MATCHY_AMD_TRACE") != nullptr;
        const auto t0 = std::chrono::steady_clock::now();
        auto ms = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
        auto db = std::make_unique<Db>();
        db->img = std::make_shared<DbImage>();
        std::string err;
        if (!db->img->open(std::move(bytes), err)) { set_error(err); return nullptr; }
        db->format = db->img->format_name();
        if (trace) fprintf(stderr, "[matchy_amd] open: parsed and checked after %.1f ms\n", ms());
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
            set_error("matchy_amd: no HIP device available (scans and extraction run on the GPU only; a handle is not opened without one)");
            return nullptr;
        }
        // "uploaded once to device memory" at open. One process per GPU selects its device with MATCHY_AMD_DEVICE.
        int dev0 = 0;
        if (const char* e = getenv("MATCHY_AMD_DEVICE")) dev0 = atoi(e);
        if (dev0 < 0 || dev0 >= ndev) { set_error("MATCHY_AMD_DEVICE out of range"); return nullptr; }
        db->default_device = dev0;
        if (trace) { (void)hipSetDevice(dev0); (void)hipFree(nullptr); fprintf(stderr, "[matchy_amd] open: HIP runtime up after %.1f ms\n", ms()); }
        db->device_db(dev0);
        if (trace) fprintf(stderr, "[matchy_amd] open: uploaded after %.1f ms\n", ms());
        return reinterpret_cast<matchy_t*>(db.release());
    } catch (const HipError& e) { set_error(e.what); return nullptr; }
    catch (const std::exception& e) { set_error(e.what()); return nullptr; }
}

static_assert(sizeof(matchy_scan_ip4_hit_t) == sizeof(uint2) && MATCHY_SCAN_IP4_DATA_BITS == C4_DATA_BITS && MATCHY_ITEM_TYPE_IPV4 == IT_IPV4, "compact record layout");
static_assert(sizeof(FinalHit) == sizeof(matchy_scan_hit_t) && sizeof(FinalHit) == 16 && offsetof(FinalHit, value) == offsetof(matchy_scan_hit_t, value) &&
                  offsetof(FinalHit, n_ids) == offsetof(matchy_scan_hit_t, n_ids) && offsetof(FinalHit, kind) == offsetof(matchy_scan_hit_t, kind),
              "pack_record writes matchy_scan_hit_t records directly");

// the internal block of a result, created where its arrays are borrowed
ScanResultInternal* internal_of(matchy_scan_result_t* out) {
    if (!out->_internal) out->_internal = new ScanResultInternal();
    return reinterpret_cast<ScanResultInternal*>(out->_internal);
}

// Hand the dense records to the caller. borrowed=true: pointers go straight to the scanner's pinned buffers (no per-hit host work at all);
// otherwise the arrays are copied into the result (canonical order is produced on the GPU, sort_hits.hip: the copy keeps it).
void fill_result(const FinalHit* fin, size_t n_fin, const uint32_t* ids, const long long* offs, size_t n_ids, uint64_t lines, uint64_t cands, uint64_t bytes, bool borrowed,
                 matchy_scan_result_t* out) {
    memset(out, 0, sizeof(*out));
    out->lines = lines; out->candidates = cands; out->bytes = bytes;
    out->n_hits = n_fin; out->n_ids = n_ids;
    if (borrowed) {
        out->hits = reinterpret_cast<const matchy_scan_hit_t*>(fin);
        out->pattern_ids = ids;
        out->data_offsets = reinterpret_cast<const int64_t*>(offs);
        return;
    }
    ScanResultInternal* in = internal_of(out);
    in->hits.resize(n_fin);
    if (n_fin) memcpy(in->hits.data(), fin, n_fin * sizeof(FinalHit));
    in->ids.assign(ids, ids + n_ids);
    in->offs.assign(offs, offs + n_ids);
    out->hits = in->hits.data();
    out->pattern_ids = in->ids.data(); out->data_offsets = in->offs.data();
}

// What a fetch mode asks for, decoded once. The arrays a result hands out all lie in one place: device memory, the scanner's pinned
// blocks (borrowed: no per-hit host work at all), or copies the result owns.
enum class Placement { DEVICE, BORROWED, OWNED };
struct FetchPlan {
    bool records, sorted, device, compact;
    explicit FetchPlan(uint32_t fetch_mode)
        : records(fetch_mode & 1u), sorted(fetch_mode & 2u), device((fetch_mode & 7u) == MATCHY_SCAN_FETCH_DEVICE),
          // MATCHY_SCAN_FETCH_COMPACT only means something for unsorted host-resident records
          compact((fetch_mode & MATCHY_SCAN_FETCH_COMPACT) && (fetch_mode & 7u) == MATCHY_SCAN_FETCH_HITS) {}
    // which fetches render and gather hit lines: those that hand records out (on the host or on the device), not a counts-only fetch
    bool renders() const { return records || device; }
    HitMode hit_mode() const { return records ? HITS_FINAL : HITS_NONE; }
    Placement placement() const { return device ? Placement::DEVICE : sorted ? Placement::OWNED : Placement::BORROWED; }
};

static_assert(sizeof(LineRec) == sizeof(matchy_scan_line_t) && offsetof(LineRec, line_end) == offsetof(matchy_scan_line_t, line_end), "k_line_resolve writes matchy_scan_line_t records directly");

// Line context of a scan_device / wait result: the result gets (or keeps) its internal block; the arrays follow the hit arrays of the
// same result — device pointers, the scanner's pinned block, or an owned copy.
void attach_lines(Scanner& sc, const ScanOutput& so, Placement at, matchy_scan_result_t* out) {
    if (!so.has_lines) return;
    ScanResultInternal* in = internal_of(out);
    in->has_lines = true;
    in->lines_with_matches = so.lines_with_matches;
    if (at == Placement::DEVICE) {
        in->lines = out->n_hits ? reinterpret_cast<const matchy_scan_line_t*>(sc.device_lines()) : nullptr;
    } else if (at == Placement::OWNED) {
        if (so.fin_lines) in->lines_own.assign(reinterpret_cast<const matchy_scan_line_t*>(so.fin_lines), reinterpret_cast<const matchy_scan_line_t*>(so.fin_lines) + so.n_fin);
        in->lines = in->lines_own.empty() ? nullptr : in->lines_own.data();
    } else {
        in->lines = reinterpret_cast<const matchy_scan_line_t*>(so.fin_lines);
        in->ip4_lines = reinterpret_cast<const matchy_scan_line_t*>(so.c4_lines);
    }
}

// The request of a lookup scan of [ptr, ptr + len) on `stream` for a fetch plan, with whole lines, segments and render armed. The hit-lines
// setting turns line context on for the scan, and a fetch that hands out no records (MATCHY_SCAN_FETCH_COUNTS) gathers nothing; the
// setting is returned for finish_result. fork: the entry forks the scan into slices() (one batch in flight; ScanRequest::fork).
// behind_gz: the scan shares the stream of the inflate kernels, and whole lines were armed (or refused) in front of them.
bool build_request(Scanner& sc, const FetchPlan& plan, const uint8_t* ptr, size_t len, hipStream_t stream, bool fork, bool behind_gz, ScanRequest& rq) {
    rq.ptr = ptr; rq.len = (uint32_t)len; rq.lookup = true;
    rq.host_mirror = plan.records && !plan.sorted; rq.compact = plan.compact;
    if (fork) { rq.fork = true; rq.slices = sc.slices(); }
    rq.lines = sc.line_context() || sc.hit_lines();
    rq.hit_lines = sc.hit_lines() && plan.renders();
    if (!behind_gz) sc.arm_whole_lines(rq);
    sc.arm_segments(len, stream);
    sc.arm_render(rq, plan.renders(), stream);
    return sc.hit_lines();
}

// The rendered block of a result whose scan was armed: it follows the hit arrays of the same result.
void attach_render(const ScanOutput& so, Placement at, matchy_scan_result_t* out) {
    if (!so.render.armed) return;
    ScanResultInternal* in = internal_of(out);
    in->has_render = true;
    in->render_status = (int32_t)so.render.status;
    in->render_len = so.render.len;
    in->render_text = so.render.text;
    if (at == Placement::OWNED && so.render.text) { in->render_own.assign(so.render.text, so.render.text + so.render.len); in->render_text = in->render_own.data(); }
}

// Hit lines of a result (`wanted`: the setting of its scan): the block and its arrays follow the hit arrays of the same result — device
// pointers, the scanner's pinned blocks, or an owned copy. A scan that gathered nothing answers with the count alone.
void attach_hit_lines(const ScanOutput& so, bool wanted, Placement at, matchy_scan_result_t* out) {
    if (!wanted) return;
    ScanResultInternal* in = internal_of(out);
    in->has_hit_lines = true;
    matchy_scan_hit_lines_t& h = in->hit_lines;
    h = matchy_scan_hit_lines_t{};
    h.n_lines = (uint32_t)so.lines_with_matches;
    if (!so.has_hit_lines) return;
    const HitLinesView& v = so.hit_lines;
    h.text = v.text; h.text_len = v.text_len; h.n_lines = v.n_lines;
    h.line_off = v.line_off; h.line_no = v.line_no; h.line_of_hit = v.line_of_fin; h.line_of_ip4_hit = v.line_of_c4;
    if (at != Placement::OWNED) return;   // an owned result has no compact records
    if (v.text_len) in->hl_text_own.assign(v.text, v.text + v.text_len);
    h.text = in->hl_text_own.empty() ? nullptr : in->hl_text_own.data();
    const size_t n_hits = v.line_of_fin ? out->n_hits : 0;
    in->hl_index_own.reserve((size_t)2 * v.n_lines + 1 + n_hits);
    in->hl_index_own.assign(v.line_off, v.line_off + v.n_lines + 1);
    if (v.n_lines) in->hl_index_own.insert(in->hl_index_own.end(), v.line_no, v.line_no + v.n_lines);
    if (n_hits) in->hl_index_own.insert(in->hl_index_own.end(), v.line_of_fin, v.line_of_fin + n_hits);
    const uint32_t* w = in->hl_index_own.data();
    h.line_off = w; h.line_no = v.n_lines ? w + v.n_lines + 1 : nullptr; h.line_of_hit = n_hits ? w + 2 * (size_t)v.n_lines + 1 : nullptr;
    h.line_of_ip4_hit = nullptr;
}

static_assert(sizeof(SegmentRec) == sizeof(matchy_scan_segment_t) && offsetof(SegmentRec, lines_with_matches) == offsetof(matchy_scan_segment_t, lines_with_matches),
              "k_seg_build writes matchy_scan_segment_t records directly");

// Segments of a result: the table is copied into the result's internal block (created when the arrays are borrowed); the per-record
// indices are device pointers, the scanner's pinned block, or an owned copy, like the hit arrays of the same result.
void attach_segments(Scanner& sc, const ScanOutput& so, Placement at, matchy_scan_result_t* out) {
    if (!so.has_segments) return;
    ScanResultInternal* in = internal_of(out);
    in->has_segments = true;
    const matchy_scan_segment_t* t = reinterpret_cast<const matchy_scan_segment_t*>(so.segments);
    in->segments.assign(t, t + so.n_segments);
    if (at == Placement::DEVICE) {
        in->segment_of_hit = out->n_hits ? sc.device_segment_of() : nullptr;
    } else if (at == Placement::OWNED) {
        if (so.seg_of_fin) in->segment_of_own.assign(so.seg_of_fin, so.seg_of_fin + out->n_hits);   // one per record of the result (scan_host gathers them itself)
        in->segment_of_hit = in->segment_of_own.empty() ? nullptr : in->segment_of_own.data();
    } else {
        in->segment_of_hit = so.seg_of_fin;
        in->segment_of_ip4_hit = so.seg_of_c4;
    }
}

// The result of a fetched scan of `bytes` bytes: the records where the plan places them, and what the scan attached to them.
// hit_lines: the scanner's setting when the scan was queued (build_request).
void finish_result(Scanner& sc, const FetchPlan& plan, const ScanOutput& so, uint64_t bytes, bool hit_lines, matchy_scan_result_t* out) {
    if (plan.device) {   // the records stay where the lookup kernel wrote them (device memory); only the counters come back
        memset(out, 0, sizeof(*out));
        out->lines = so.lines; out->candidates = so.n_cand; out->bytes = bytes;
        out->n_hits = so.n_hits; out->n_ids = sc.device_final_id_count();
        out->hits = reinterpret_cast<const matchy_scan_hit_t*>(sc.device_final());
        out->pattern_ids = sc.device_final_ids();
        out->data_offsets = reinterpret_cast<const int64_t*>(sc.device_final_offs());
        internal_of(out)->on_device = true;   // marks the residency: host-side readers of the result refuse device pointers
    } else {
        fill_result(so.fin, so.n_fin, so.fin_ids, so.fin_offs, so.n_fin_ids, so.lines, so.n_cand, bytes, !plan.sorted, out);
        out->ip4_hits = reinterpret_cast<const matchy_scan_ip4_hit_t*>(so.c4); out->n_ip4_hits = so.n_c4;
        if (!plan.records) out->n_hits = so.n_hits;  // count only; `hits` stays NULL
    }
    const Placement at = plan.placement();
    attach_lines(sc, so, at, out);
    attach_segments(sc, so, at, out);
    attach_hit_lines(so, hit_lines, at, out);
    attach_render(so, at, out);
}

}  // namespace

int mxy::capi::default_device_of(const matchy_t* db) { return reinterpret_cast<const Db*>(db)->default_device; }
const char* mxy::capi::gz_window_refusal(const uint8_t* packed, size_t packed_len, const matchy_gz_window_t* w) {
    if (!packed || packed_len == 0) return "no members (packed_len is 0)";
    if (!w) return "no window";
    if (w->flags & ~MATCHY_WINDOW_LAST) return "unknown flag bits";
    if (w->carry_len > w->carry_cap) return "carry_len is above carry_cap";
    if (!w->carry && w->carry_len) return "carry is NULL with a carry_len above 0";
    if (w->carry_cap >= (1u << 31) || packed_len > 0xFFFFFFFFull) return "the batch reaches 2^31 bytes";
    return nullptr;
}
const char* mxy::capi::gz_stream_refusal(const uint8_t* packed, size_t packed_len, const matchy_gz_stream_window_t* w) {
    if (!packed || packed_len == 0) return "no compressed bytes (packed_len is 0)";
    if (packed_len > 0xFFFFFFFFull) return "a window holds less than 4 GiB of compressed bytes";
    if (!w) return "no window";
    if (w->flags & ~(MATCHY_STREAM_FIRST | MATCHY_STREAM_FILE_END)) return "unknown flag bits";
    if (w->carry_len > w->carry_cap) return "carry_len is above carry_cap";
    if (!w->carry && w->carry_len) return "carry is NULL with a carry_len above 0";
    if (w->text_cap == 0) return "text_cap is 0";
    if ((uint64_t)w->carry_len + w->text_cap + 1 >= 0x7FFF0000ull || w->carry_cap >= (1u << 31)) return "the batch reaches 2^31 bytes (carry_len + text_cap)";
    if (!(w->flags & MATCHY_STREAM_FIRST)) {
        if (!w->state) return "no state (only a window with MATCHY_STREAM_FIRST has none)";
        if (w->state->bit > 7) return "state: bit is above 7";
        if (w->state->history_len > 32768 || w->state->history_len > w->state->text_bytes) return "state: history_len is above 32768 or above text_bytes";
    }
    return nullptr;
}

const char* mxy::capi::utf16_refusal(const uint8_t* data, size_t len, uint32_t byte_order) {
    if (!data && len) return "no input";
    if (byte_order > MATCHY_UTF16_BE) return "byte_order is MATCHY_UTF16_LE or MATCHY_UTF16_BE";
    if (len >= ((size_t)1 << 31) || utf16::out_bound(len) >= (1ull << 31)) return "the input may transcode to 2^31 bytes or more (3 bytes per code unit); cut it into smaller batches";
    return nullptr;
}
const char* mxy::capi::unescape_refusal(const uint8_t* data, size_t len, uint32_t modes) {
    if (modes == 0 || modes > (MATCHY_UNESCAPE_PERCENT | MATCHY_UNESCAPE_JSON)) return "modes is MATCHY_UNESCAPE_PERCENT, MATCHY_UNESCAPE_JSON or both";
    if (!data && len) return "no input";
    if (len >= 0x7FFF0000u) return "the input reaches 2^31 bytes; cut it into smaller batches";
    return nullptr;
}

// Scans behind a front pass (Scanner::utf16_transcode, Scanner::unescape): the pass and the scan are queued on the scanner's own
// stream; the fetch is that of matchy_scanner_scan_device. scan_front_text is what the entries share: the scan of the text `b` the pass
// left on the device, queue_text() behind the scan's kernels, finish() behind the fetch (the pass's Result, which it returns), and the
// text in the result — borrowed, or owned where the hit arrays are.
namespace {
template <class QueueText, class Finish>
auto scan_front_text(ScannerH* h, const Scanner::GzBatch& b, uint32_t fetch_mode, const char* entry, QueueText&& queue_text, Finish&& finish,
                     matchy_scan_result_t* out) {
    if (b.len >= 0x7FFF0000u) throw ParamError{std::string(entry) + ": the text reaches 2^31 bytes; cut the input into smaller batches"};
    const FetchPlan plan(fetch_mode);
    ScanRequest rq;   // not forked: the scan shares the stream of the pass in front of it
    const bool hit_lines = build_request(*h->sc, plan, b.text, b.len, b.stream, false, true, rq);
    h->sc->scan_device(rq, b.stream);
    queue_text();
    ScanOutput so;
    h->sc->fetch(so, false, b.stream, plan.hit_mode(), plan.sorted);
    const auto u = finish();
    finish_result(*h->sc, plan, so, u.text_len, hit_lines, out);
    ScanResultInternal* in = internal_of(out);
    in->front_text = u.text; in->front_text_len = u.text_len;
    if (plan.sorted && u.text) { in->front_text_own.assign(u.text, u.text + u.text_len); in->front_text = in->front_text_own.data(); }
    return u;
}
}  // namespace

// hit tally (Scanner::set_tally, tally.hip): the table is the scanner's
namespace {
struct TallyInternal {
    std::vector<TallyEntry> rows;
    std::vector<matchy_tally_entry_t> entries;
};
}  // namespace
bool mxy::capi::scanner_tally_top(matchy_scanner_t* s, size_t limit, std::vector<TallyEntry>& rows, uint64_t& distinct, uint64_t& matches) {
    Scanner& sc = *reinterpret_cast<ScannerH*>(s)->sc;
    rows.clear();
    if (!sc.hit_tally()) return false;
    sc.tally_top(limit, rows);
    distinct = sc.hit_tally()->distinct(); matches = sc.hit_tally()->matches();
    return true;
}
void mxy::capi::fill_tally(std::vector<TallyEntry>&& rows, uint64_t distinct, uint64_t matches, matchy_tally_t* out) {
    auto in = std::make_unique<TallyInternal>();
    in->rows = std::move(rows);
    in->entries.resize(in->rows.size());
    for (size_t i = 0; i < in->rows.size(); ++i) {
        const TallyEntry& r = in->rows[i];
        in->entries[i] = matchy_tally_entry_t{reinterpret_cast<const uint8_t*>(r.text.data()), (uint32_t)r.text.size(), r.item_type, r.count};
    }
    out->entries = in->entries.empty() ? nullptr : in->entries.data();
    out->n_entries = in->entries.size();
    out->distinct = distinct; out->matches = matches;
    out->_internal = in.release();
}

extern "C" {

const char* matchy_amd_last_error(void) { return g_last_error.c_str(); }
int32_t matchy_amd_ac_dfa_states(const matchy_t* db_) {
    if (!db_) return -1;
    Db* db = const_cast<Db*>(reinterpret_cast<const Db*>(db_));
    try {
        std::lock_guard<std::mutex> lk(db->mu);
        return (int32_t)std::min<uint32_t>(db->device_db(db->default_device)->view.dfa ? db->device_db(db->default_device)->view.dfa_states : 0u, 0x7FFFFFFFu);
    } catch (...) { return -1; }
}
int32_t matchy_amd_suffix_filter(const matchy_t* db_) {
    if (!db_) return -1;
    Db* db = const_cast<Db*>(reinterpret_cast<const Db*>(db_));
    try {
        std::lock_guard<std::mutex> lk(db->mu);
        return db->device_db(db->default_device)->view.sfx_bm ? 1 : 0;
    } catch (...) { return -1; }
}
void* matchy_amd_pinned_alloc(size_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); set_error("matchy_amd_pinned_alloc: hipHostMalloc failed"); return nullptr; }
    return p;
}
void matchy_amd_pinned_free(void* p) { if (p) (void)hipHostFree(p); }
int32_t matchy_amd_host_register(const void* ptr, size_t bytes) {
    if (!ptr || !bytes) return MATCHY_ERROR_INVALID_PARAM;
    return mxy::pins::add_caller(ptr, bytes) == 0 ? MATCHY_SUCCESS : MATCHY_ERROR_IO;
}
void matchy_amd_host_unregister(const void* ptr) { if (ptr) mxy::pins::remove_caller(ptr); }
int32_t matchy_amd_device_count(void) {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}
const char* matchy_version(void) { return "matchy-amd 0.1.0 (reference matchy 1.2.2 surface)"; }

// ------------------------------------------------------------------------------------------------ builder
matchy_builder_t* matchy_builder_new(void) { return reinterpret_cast<matchy_builder_t*>(new Builder()); }
void matchy_builder_free(matchy_builder_t* b) { delete reinterpret_cast<Builder*>(b); }
int32_t matchy_builder_set_case_insensitive(matchy_builder_t* b, bool ci) {
    if (!b) return MATCHY_ERROR_INVALID_PARAM;
    reinterpret_cast<Builder*>(b)->b.set_case_insensitive(ci);
    return MATCHY_SUCCESS;
}
int32_t matchy_builder_set_build_epoch(matchy_builder_t* b, uint64_t epoch) {
    if (!b) return MATCHY_ERROR_INVALID_PARAM;
    reinterpret_cast<Builder*>(b)->b.set_build_epoch(epoch);
    return MATCHY_SUCCESS;
}
int32_t matchy_builder_add(matchy_builder_t* b, const char* key, const char* json_data) {
    if (!b || !key || !json_data) return MATCHY_ERROR_INVALID_PARAM;
    DataValue v;
    std::string err;
    if (!parse_json(json_data, strlen(json_data), NumberTyping::SERDE, v, err)) { set_error(err); return MATCHY_ERROR_INVALID_FORMAT; }
    if (v.type != DataValue::MAP) {  // single value: wrapped as {"value": v} (c_api/matchy.rs:427-435)
        DataValue m = DataValue::Map();
        m.map["value"] = std::move(v);
        v = std::move(m);
    }
    Builder* bb = reinterpret_cast<Builder*>(b);
    if (!bb->b.add_entry(key, v)) { set_error(bb->b.error()); return MATCHY_ERROR_INVALID_FORMAT; }
    return MATCHY_SUCCESS;
}
int32_t matchy_builder_set_description(matchy_builder_t* b, const char* description) {
    if (!b || !description) return MATCHY_ERROR_INVALID_PARAM;
    reinterpret_cast<Builder*>(b)->b.set_description("en", description);
    return MATCHY_SUCCESS;
}
int32_t matchy_builder_build(matchy_builder_t* b, uint8_t** buffer, uintptr_t* size) {
    if (!b || !buffer || !size) return MATCHY_ERROR_INVALID_PARAM;
    Builder* bb = reinterpret_cast<Builder*>(b);
    std::vector<uint8_t> out;
    if (!bb->b.build(out)) { set_error(bb->b.error()); return MATCHY_ERROR_INVALID_FORMAT; }
    uint8_t* p = (uint8_t*)malloc(out.size() ? out.size() : 1);
    if (!p) return MATCHY_ERROR_OUT_OF_MEMORY;
    memcpy(p, out.data(), out.size());
    *buffer = p;
    *size = out.size();
    return MATCHY_SUCCESS;
}
int32_t matchy_builder_save(matchy_builder_t* b, const char* filename) {
    if (!b || !filename) return MATCHY_ERROR_INVALID_PARAM;
    Builder* bb = reinterpret_cast<Builder*>(b);
    std::vector<uint8_t> out;
    if (!bb->b.build(out)) { set_error(bb->b.error()); return MATCHY_ERROR_INVALID_FORMAT; }
    FILE* f = fopen(filename, "wb");
    if (!f) return MATCHY_ERROR_IO;
    bool ok = fwrite(out.data(), 1, out.size(), f) == out.size();
    ok = fclose(f) == 0 && ok;
    return ok ? MATCHY_SUCCESS : MATCHY_ERROR_IO;
}

// ------------------------------------------------------------------------------------------------ open / close
void matchy_init_open_options(matchy_open_options_t* o) {
    if (!o) return;
    o->cache_capacity = 10000; o->auto_reload = false; o->reload_callback = nullptr; o->reload_callback_user_data = nullptr;
}
matchy_t* matchy_open(const char* filename) {
    if (!filename) return nullptr;
    std::vector<uint8_t> bytes;
    if (!read_file(filename, bytes)) { set_error(std::string("Failed to open ") + filename); return nullptr; }
    return open_bytes(std::move(bytes));
}
matchy_t* matchy_open_with_options(const char* filename, const matchy_open_options_t* options) {
    if (!filename || !options) return nullptr;
    matchy_t* db = matchy_open(filename);
    if (db) reinterpret_cast<Db*>(db)->cache_cap = options->cache_capacity;   // 0 disables the query cache (c_api/matchy.rs:805-808)
    return db;
}
matchy_t* matchy_open_buffer(const uint8_t* buffer, uintptr_t size) {
    if (!buffer || size == 0) return nullptr;
    return open_bytes(std::vector<uint8_t>(buffer, buffer + size));
}
void matchy_close(matchy_t* db) { delete reinterpret_cast<Db*>(db); }

const char* matchy_format(const matchy_t* db) { return db ? reinterpret_cast<const Db*>(db)->format.c_str() : nullptr; }
bool matchy_has_ip_data(const matchy_t* db) { return db && reinterpret_cast<const Db*>(db)->img->has_ip; }
bool matchy_has_literal_data(const matchy_t* db) { return db && reinterpret_cast<const Db*>(db)->img->has_literal; }
bool matchy_has_glob_data(const matchy_t* db) { return db && reinterpret_cast<const Db*>(db)->img->has_glob; }
bool matchy_has_string_data(const matchy_t* db) { return matchy_has_literal_data(db) || matchy_has_glob_data(db); }
bool matchy_has_pattern_data(const matchy_t* db) { return matchy_has_string_data(db); }

void matchy_get_stats(const matchy_t* dbc, matchy_stats_t* st) {
    if (!dbc || !st) return;
    const Db* db = reinterpret_cast<const Db*>(dbc);
    *st = matchy_stats_t{db->st_total.load(), db->st_match.load(), db->st_nomatch.load(), db->st_chit.load(), db->st_cmiss.load(), db->st_ip.load(),
                         db->st_str.load()};
}
void matchy_clear_cache(const matchy_t* dbc) {
    if (!dbc) return;
    Db* db = const_cast<Db*>(reinterpret_cast<const Db*>(dbc));
    db->cache().clear();   // the calling thread's cache, like Database::clear_cache (thread-local caches)
}
uintptr_t matchy_pattern_count(const matchy_t* db) { return db ? reinterpret_cast<const Db*>(db)->img->pattern_count : 0; }
char* matchy_metadata(const matchy_t* db) {
    if (!db) return nullptr;
    std::string s;
    to_json(reinterpret_cast<const Db*>(db)->img->metadata, s);
    return strdup(s.c_str());
}
char* matchy_get_pattern_string(const matchy_t* db, uint32_t id) {
    if (!db) return nullptr;
    const DbImage& img = *reinterpret_cast<const Db*>(db)->img;
    if (!img.has_glob || id >= img.pattern_count) return nullptr;
    return strdup(img.pattern_string(id).c_str());
}
void matchy_free_string(char* s) { free(s); }

// ------------------------------------------------------------------------------------------------ single query
// Database::lookup (database.rs:725-804): a query that parses as an IP address takes the trie, anything else the string
// path. Fills the one-candidate "scan" both single-query entries run through the lookup kernels. False: query too long.
static bool query_candidate(const char* query, size_t qn, IpAddr& ip, bool& is_ip, std::string& text, Candidate& c) {
    text.assign(query, qn);
    c = Candidate{0, 0, 0, 0};
    is_ip = parse_ip(query, qn, ip);
    if (is_ip) {
        if (!ip.v6) {
            c.v4 = ((uint32_t)ip.b[0] << 24) | ((uint32_t)ip.b[1] << 16) | ((uint32_t)ip.b[2] << 8) | ip.b[3];
            c.len_type = (uint32_t)qn | ((uint32_t)IT_IPV4 << 24);
        } else {
            char buf[64];
            snprintf(buf, sizeof(buf), "%x:%x:%x:%x:%x:%x:%x:%x", (ip.b[0] << 8) | ip.b[1], (ip.b[2] << 8) | ip.b[3], (ip.b[4] << 8) | ip.b[5],
                     (ip.b[6] << 8) | ip.b[7], (ip.b[8] << 8) | ip.b[9], (ip.b[10] << 8) | ip.b[11], (ip.b[12] << 8) | ip.b[13], (ip.b[14] << 8) | ip.b[15]);
            text = buf;
            c.len_type = (uint32_t)text.size() | ((uint32_t)IT_IPV6 << 24);
        }
        return true;
    }
    if (qn >= (1u << 24)) return false;
    c.len_type = (uint32_t)qn | ((uint32_t)IT_DOMAIN << 24);
    return true;
}

// One uncached query. SURVEY §8b: single queries stay on the CPU (latency) — host_lookup.cpp walks the same sections the kernels get
// uploaded; MATCHY_AMD_QUERY_ON_GPU=1 sends the query through the lookup kernels instead (the GPU tests hold the two against each other
// and against the oracle). Fills `so` like Scanner::lookup_one: no hit, or hits[0] (+ its glob ids in so.ids).
// Takes no lock on the host path (the sections are read-only: queries of several threads proceed side by side, like the reference's
// per-thread lookups); the kernel path serialises on Db::mu.
static void single_lookup(Db* db, const std::string& text, const Candidate& c, const IpAddr& ip, bool is_ip, ScanOutput& so) {
    static const bool on_gpu = [] { const char* e = getenv("MATCHY_AMD_QUERY_ON_GPU"); return e && atoi(e) != 0; }();
    if (on_gpu) {
        std::lock_guard<std::mutex> lk(db->mu);
        if (!db->query_scanner) db->query_scanner = std::make_unique<Scanner>(db->img, db->device_db(db->default_device), EX_ALL, 2);
        db->query_scanner->lookup_one(text, c, so);
        return;
    }
    std::call_once(db->host_tables_once, [db] { db->host_tables = std::make_unique<HostTables>(*db->img); });
    HostHit hh;
    host_lookup(*db->img, *db->host_tables, text, is_ip ? &ip : nullptr, hh);
    so.hits.clear(); so.ids.clear();
    if (!hh.kind) return;
    if (hh.globs.size() > 0xFFFFu) throw std::runtime_error("query matches more than 65535 glob patterns");   // the limit of the scan records (engine.cpp)
    Hit h{};
    h.kind = hh.kind; h.prefix_len = hh.prefix_len; h.a = hh.a; h.ids_off = 0; h.n_globs = (uint16_t)hh.globs.size();
    h.start = 0; h.len_type = c.len_type;
    so.hits.push_back(h);
    so.ids = std::move(hh.globs);
}

void matchy_query_into(const matchy_t* dbc, const char* query, matchy_result_t* result) {
    if (!result) return;
    *result = matchy_result_t{false, 0, nullptr, nullptr};
    if (!dbc || !query) return;
    Db* db = const_cast<Db*>(reinterpret_cast<const Db*>(dbc));
    size_t qn = strlen(query);
    if (!valid_utf8_host((const uint8_t*)query, qn)) return;  // CStr::to_str failure -> found=false
    try {
        const std::string key(query, qn);
        Db::Lru& cache = db->cache();
        IpAddr ip;
        bool is_ip;
        std::string text;
        Candidate c;
        if (const Db::Cached* hit = db->cache_cap ? cache.get(key) : nullptr) {
            // cache hit (database.rs:727-757): same accounting as a lookup, except that a cached miss is typed by parsing the query
            db->st_total++; db->st_chit++;
            if (hit->kind == 0) { if (parse_ip(query, qn, ip)) db->st_ip++; else db->st_str++; db->st_nomatch++; return; }
            if (hit->kind == 2) db->st_ip++; else db->st_str++;
            db->st_match++;
            if (!hit->has_data) return;
            result->found = true; result->prefix_len = hit->prefix_len;
            result->_data_cache = new DataValue(hit->data);
            result->_db_ref = dbc;
            return;
        }
        if (!query_candidate(query, qn, ip, is_ip, text, c)) return;
        ScanOutput so;
        single_lookup(db, text, c, ip, is_ip, so);
        db->st_total++;
        if (db->cache_cap) db->st_cmiss++;
        if (so.hits.empty()) {   // a miss counts as a string query (database.rs:786-790)
            db->st_str++; db->st_nomatch++;
            cache.put(key, Db::Cached{0, 0, false, DataValue()}, db->cache_cap);
            return;
        }
        const Hit& h = so.hits[0];
        if (h.kind == 2) db->st_ip++; else db->st_str++;
        db->st_match++;
        DataValue* dv = new DataValue();
        bool ok = false;
        if (h.kind == 2) { ok = db->img->decode_data(h.a, *dv); result->prefix_len = h.prefix_len; }
        else {
            // first pattern's data only (c_api/matchy.rs:1143-1154)
            uint32_t off;
            bool have = false;
            if (h.a != 0xFFFFFFFFu && db->img->lit_data_offset(h.a, off)) have = true;
            else if ((h.a == 0xFFFFFFFFu || !db->img->lit_data_offset(h.a, off)) && h.n_globs > 0) have = db->img->glob_data_offset(so.ids[h.ids_off], off);
            ok = have && db->img->decode_data(off, *dv);
        }
        if (!ok) { delete dv; result->prefix_len = 0; cache.put(key, Db::Cached{h.kind, 0, false, DataValue()}, db->cache_cap); return; }
        result->found = true;
        result->_data_cache = dv;
        result->_db_ref = dbc;
        cache.put(key, Db::Cached{h.kind, result->prefix_len, true, *dv}, db->cache_cap);
    } catch (const HipError& e) { set_error(e.what); }
    catch (const std::exception& e) { set_error(e.what()); }
}
// The answer `matchy query DB QUERY` prints (bin/commands/query_cmd.rs:8-69), as compact JSON: an array with one object per
// pattern that carries data (literal first, then globs by id), or one object for an IP hit (its data plus "cidr" and
// "prefix_len"), or [] when nothing matches. *found follows the command's exit status rule (:19-21).
char* matchy_amd_query_json(const matchy_t* dbc, const char* query, int32_t* found) {
    if (found) *found = 0;
    if (!dbc || !query) return nullptr;
    Db* db = const_cast<Db*>(reinterpret_cast<const Db*>(dbc));
    const size_t qn = strlen(query);
    if (!valid_utf8_host((const uint8_t*)query, qn)) return strdup("[]");
    try {
        IpAddr ip;
        bool is_ip;
        std::string text;
        Candidate c;
        if (!query_candidate(query, qn, ip, is_ip, text, c)) return strdup("[]");
        ScanOutput so;
        single_lookup(db, text, c, ip, is_ip, so);
        if (so.hits.empty()) return strdup("[]");
        const Hit& h = so.hits[0];
        if (found) *found = 1;
        std::string o = "[";
        if (h.kind == 2) {
            DataValue dv;
            if (!db->img->decode_data(h.a, dv)) { set_error("query: cannot decode the data record"); return nullptr; }
            if (dv.type == DataValue::MAP) {
                dv.map["cidr"] = DataValue::String(format_cidr(ip, h.prefix_len));
                dv.map["prefix_len"] = DataValue::Uint16(h.prefix_len);
            }
            to_json(dv, o);
        } else {
            bool any = false;
            auto push = [&](uint32_t off) {
                DataValue dv;
                if (!db->img->decode_data(off, dv)) return;
                if (any) o.push_back(',');
                to_json(dv, o);
                any = true;
            };
            uint32_t off;
            if (h.a != 0xFFFFFFFFu && db->img->lit_data_offset(h.a, off)) push(off);
            for (uint32_t k = 0; k < h.n_globs; ++k) if (db->img->glob_data_offset(so.ids[h.ids_off + k], off)) push(off);
        }
        o.push_back(']');
        return strdup(o.c_str());
    } catch (const HipError& e) { set_error(e.what); }
    catch (const std::exception& e) { set_error(e.what()); }
    return nullptr;
}
matchy_result_t matchy_query(const matchy_t* db, const char* query) {
    matchy_result_t r;
    matchy_query_into(db, query, &r);
    return r;
}
void matchy_free_result(matchy_result_t* r) {
    if (!r) return;
    delete reinterpret_cast<DataValue*>(r->_data_cache);
    r->_data_cache = nullptr;
}
char* matchy_result_to_json(const matchy_result_t* r) {
    if (!r || !r->found || !r->_data_cache) return nullptr;
    std::string s;
    to_json(*reinterpret_cast<const DataValue*>(r->_data_cache), s);
    return strdup(s.c_str());
}

// ------------------------------------------------------------------------------------------------ structured data
namespace {
matchy_entry_data_t entry_empty() {
    matchy_entry_data_t e;
    memset(&e, 0, sizeof(e));
    return e;
}
// matchy_entry_data_t::from_data_value (c_api/matchy.rs:1599-1690)
matchy_entry_data_t entry_from(const DataValue& v) {
    matchy_entry_data_t e = entry_empty();
    e.has_data = true;
    e.type_ = (uint32_t)v.type;
    switch (v.type) {
        case DataValue::POINTER: e.value.pointer = (uint32_t)v.u; break;
        case DataValue::STRING: e.value.utf8_string = v.str.c_str(); e.data_size = (uint32_t)v.str.size(); break;
        case DataValue::DOUBLE: e.value.double_value = v.f64; e.data_size = 8; break;
        case DataValue::BYTES: e.value.bytes = (const uint8_t*)v.str.data(); e.data_size = (uint32_t)v.str.size(); break;
        case DataValue::UINT16: e.value.uint16 = (uint16_t)v.u; e.data_size = 2; break;
        case DataValue::UINT32: e.value.uint32 = (uint32_t)v.u; e.data_size = 4; break;
        case DataValue::MAP: e.data_size = (uint32_t)v.map.size(); break;
        case DataValue::INT32: e.value.int32 = v.i32; e.data_size = 4; break;
        case DataValue::UINT64: e.value.uint64 = v.u; e.data_size = 8; break;
        case DataValue::UINT128:
            for (int i = 0; i < 8; ++i) { e.value.uint128[i] = (uint8_t)(v.uhi >> (56 - 8 * i)); e.value.uint128[8 + i] = (uint8_t)(v.u >> (56 - 8 * i)); }
            e.data_size = 16;
            break;
        case DataValue::ARRAY: e.data_size = (uint32_t)v.arr.size(); break;
        case DataValue::BOOL: e.value.boolean = v.u != 0; e.data_size = 1; break;
        case DataValue::FLOAT: e.value.float_value = v.f32; e.data_size = 4; break;
    }
    return e;
}
const DataValue* entry_root(const matchy_entry_s* entry) {
    if (!entry || !entry->data_ptr) return nullptr;
    const matchy_result_t* r = reinterpret_cast<const matchy_result_t*>(entry->data_ptr);
    return reinterpret_cast<const DataValue*>(r->_data_cache);
}
void flatten(const DataValue& v, matchy_entry_data_list_t**& tail) {
    auto* node = new matchy_entry_data_list_t{entry_from(v), nullptr};
    *tail = node;
    tail = &node->next;
    if (v.type == DataValue::MAP) for (const auto& kv : v.map) flatten(kv.second, tail);
    else if (v.type == DataValue::ARRAY) for (const DataValue& c : v.arr) flatten(c, tail);
}
}  // namespace

int32_t matchy_result_get_entry(const matchy_result_t* result, matchy_entry_s* entry) {
    if (!result || !entry) return MATCHY_ERROR_INVALID_PARAM;
    if (!result->found) return MATCHY_ERROR_NO_DATA;
    entry->db = result->_db_ref;
    entry->data_ptr = result;
    return MATCHY_SUCCESS;
}
int32_t matchy_aget_value(const matchy_entry_s* entry, matchy_entry_data_t* out, const char* const* path) {
    if (!entry || !out || !path) return MATCHY_ERROR_INVALID_PARAM;
    for (size_t i = 0; path[i]; ++i) if (!valid_utf8_host((const uint8_t*)path[i], strlen(path[i]))) return MATCHY_ERROR_INVALID_PARAM;
    *out = entry_empty();
    const DataValue* v = entry_root(entry);
    if (!v) return MATCHY_ERROR_NO_DATA;
    for (size_t i = 0; path[i]; ++i) {   // navigate_path (c_api/matchy.rs:1692-1710)
        if (v->type == DataValue::MAP) {
            auto it = v->map.find(path[i]);
            if (it == v->map.end()) return MATCHY_ERROR_LOOKUP_PATH_INVALID;
            v = &it->second;
        } else if (v->type == DataValue::ARRAY) {
            const char* s = path[i];
            if (*s == '+') ++s;   // usize::from_str accepts a leading '+'
            if (!*s) return MATCHY_ERROR_LOOKUP_PATH_INVALID;
            size_t idx = 0;
            for (; *s; ++s) {
                if (*s < '0' || *s > '9' || idx > ((size_t)1 << 56)) return MATCHY_ERROR_LOOKUP_PATH_INVALID;
                idx = idx * 10 + (size_t)(*s - '0');
            }
            if (idx >= v->arr.size()) return MATCHY_ERROR_LOOKUP_PATH_INVALID;
            v = &v->arr[idx];
        } else {
            return MATCHY_ERROR_LOOKUP_PATH_INVALID;
        }
    }
    *out = entry_from(*v);
    return MATCHY_SUCCESS;
}
int32_t matchy_get_entry_data_list(const matchy_entry_s* entry, matchy_entry_data_list_t** list) {
    if (!entry || !list) return MATCHY_ERROR_INVALID_PARAM;
    const DataValue* v = entry_root(entry);
    if (!v) return MATCHY_ERROR_NO_DATA;
    *list = nullptr;
    matchy_entry_data_list_t** tail = list;
    flatten(*v, tail);
    return MATCHY_SUCCESS;
}
void matchy_free_entry_data_list(matchy_entry_data_list_t* list) {
    while (list) { matchy_entry_data_list_t* n = list->next; delete list; list = n; }
}

int32_t matchy_validate(const char* filename, int32_t level, char** error_message) {
    if (error_message) *error_message = nullptr;
    if (!filename || !valid_utf8_host((const uint8_t*)filename, strlen(filename))) return MATCHY_ERROR_INVALID_PARAM;
    if (level != MATCHY_VALIDATION_STANDARD && level != MATCHY_VALIDATION_STRICT) return MATCHY_ERROR_INVALID_PARAM;
    std::vector<uint8_t> bytes;
    if (!read_file(filename, bytes)) {
        if (error_message) *error_message = strdup("Failed to validate database");
        return MATCHY_ERROR_IO;
    }
    DbImage img;
    std::string err;
    if (!img.open(std::move(bytes), err)) {
        if (error_message) *error_message = strdup(err.empty() ? "Validation failed (no error details)" : err.c_str());
        return MATCHY_ERROR_CORRUPT_DATA;
    }
    return MATCHY_SUCCESS;
}
int32_t matchy_builder_set_schema(matchy_builder_t* b, const char* name) {
    if (!b || !name) return MATCHY_ERROR_INVALID_PARAM;
    return MATCHY_ERROR_UNKNOWN_SCHEMA;
}

// ------------------------------------------------------------------------------------------------ extractor
matchy_extractor_t* matchy_extractor_create(uint32_t flags) { return matchy_amd_extractor_create(flags, 2); }
// ExtractorBuilder::min_domain_labels (matchy-extractor/src/lib.rs:101-104; `matchy extract --min-labels`)
matchy_extractor_t* matchy_amd_extractor_create(uint32_t flags, uint32_t min_domain_labels) {
    try {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { set_error("matchy_amd: no HIP device available"); return nullptr; }
        auto e = std::make_unique<ExtractorH>();
        e->flags = flags;
        e->img = std::make_shared<DbImage>();  // no sections: has_ip/has_literal/has_glob all false
        e->img->node_count = 0;
        e->ddb = std::make_shared<DeviceDb>();
        int dev0 = 0;   // like matchy_open: one process per GPU selects its device with MATCHY_AMD_DEVICE
        if (const char* ev = getenv("MATCHY_AMD_DEVICE")) dev0 = atoi(ev);
        if (dev0 < 0 || dev0 >= ndev) { set_error("MATCHY_AMD_DEVICE out of range"); return nullptr; }
        e->ddb->upload(*e->img, dev0);
        e->scanner = std::make_unique<Scanner>(e->img, e->ddb, flags, min_domain_labels ? min_domain_labels : 2);
        return reinterpret_cast<matchy_extractor_t*>(e.release());
    } catch (const HipError& e) { set_error(e.what); return nullptr; }
    catch (const std::exception& e) { set_error(e.what()); return nullptr; }
}
void matchy_extractor_free(matchy_extractor_t* e) { delete reinterpret_cast<ExtractorH*>(e); }
// distinct candidate texts (Scanner::set_unique, distinct.hip): the set is the handle's, under the handle's lock
void matchy_amd_extractor_set_unique(matchy_extractor_t* ec, bool enabled) {
    if (!ec) return;
    ExtractorH* e = reinterpret_cast<ExtractorH*>(ec);
    std::lock_guard<std::mutex> lk(e->mu);
    e->scanner->set_unique(enabled);
}
bool matchy_amd_extractor_unique(const matchy_extractor_t* ec) {
    if (!ec) return false;
    ExtractorH* e = const_cast<ExtractorH*>(reinterpret_cast<const ExtractorH*>(ec));
    std::lock_guard<std::mutex> lk(e->mu);
    return e->scanner->unique();
}
void matchy_amd_extractor_reset_unique(matchy_extractor_t* ec) {
    if (!ec) return;
    ExtractorH* e = reinterpret_cast<ExtractorH*>(ec);
    std::lock_guard<std::mutex> lk(e->mu);
    try { e->scanner->reset_unique(); } catch (const HipError& ex) { set_error(ex.what); }
}
uint64_t matchy_amd_extractor_unique_count(const matchy_extractor_t* ec) {
    if (!ec) return 0;
    ExtractorH* e = const_cast<ExtractorH*>(reinterpret_cast<const ExtractorH*>(ec));
    std::lock_guard<std::mutex> lk(e->mu);
    return e->scanner->unique_count();
}
const char* matchy_item_type_name(uint8_t t) { return item_type_name(t); }

int32_t matchy_extractor_extract_chunk(const matchy_extractor_t* ec, const uint8_t* data, uintptr_t len, matchy_matches_t* out) {
    if (!ec || !out || (!data && len)) return MATCHY_ERROR_INVALID_PARAM;
    ExtractorH* e = const_cast<ExtractorH*>(reinterpret_cast<const ExtractorH*>(ec));
    try {
        std::lock_guard<std::mutex> lk(e->mu);
        ScanOutput so;
        std::vector<uint64_t> bases;
        e->scanner->scan_host(data, len, false, true, so, &bases, nullptr, nullptr, nullptr);
        size_t nc = so.cands.size();
        std::vector<uint32_t> order(nc);
        for (uint32_t i = 0; i < nc; ++i) order[i] = i;
        auto abs_start = [&](uint32_t i) { return (uint64_t)so.cands[i].start + bases[i]; };
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
            int ra = type_rank(so.cands[a].len_type >> 24), rb = type_rank(so.cands[b].len_type >> 24);
            if (ra != rb) return ra < rb;
            uint64_t sa = abs_start(a), sb = abs_start(b);
            if (sa != sb) return sa < sb;
            return (so.cands[a].len_type >> 24) < (so.cands[b].len_type >> 24);
        });
        auto* in = new MatchesInternal();
        in->values.reserve(nc);
        in->items.reserve(nc);
        for (uint32_t oi : order) {
            const Candidate& c = so.cands[oi];
            uint64_t s = abs_start(oi), n = c.len_type & 0xFFFFFF;
            uint8_t ty = (uint8_t)(c.len_type >> 24);
            std::string val;
            if (ty == IT_IPV4) {  // as_value(): canonical Display (matchy-extractor/src/lib.rs:300-311)
                uint8_t b[4] = {(uint8_t)(c.v4 >> 24), (uint8_t)(c.v4 >> 16), (uint8_t)(c.v4 >> 8), (uint8_t)c.v4};
                val = format_ipv4(b);
            } else if (ty == IT_IPV6) {
                uint8_t b[16];
                if (parse_ipv6((const char*)data + s, n, b)) val = format_ipv6(b);
            } else val.assign((const char*)data + s, n);
            in->values.push_back(std::move(val));
            in->items.push_back(matchy_match_t{ty, nullptr, (uintptr_t)s, (uintptr_t)(s + n)});
        }
        for (size_t i = 0; i < in->items.size(); ++i) in->items[i].value = in->values[i].c_str();
        out->items = in->items.data(); out->count = in->items.size(); out->_internal = in;
        return MATCHY_SUCCESS;
    } catch (const HipError& ex) { set_error(ex.what); return MATCHY_ERROR_IO; }
    catch (const std::exception& ex) { set_error(ex.what()); return MATCHY_ERROR_IO; }
}
// candidates as text (Scanner::set_extract_text, extract_render.hip): the block is the scanner's, under the handle's lock
int32_t matchy_amd_extractor_extract_rendered(const matchy_extractor_t* ec, const uint8_t* data, uintptr_t len, uint32_t format, matchy_amd_extract_text_t* out) {
    if (!ec || !out || (!data && len) || format > MATCHY_AMD_EXTRACT_FORMAT_TEXT) return MATCHY_ERROR_INVALID_PARAM;
    memset(out, 0, sizeof(*out));
    ExtractorH* e = const_cast<ExtractorH*>(reinterpret_cast<const ExtractorH*>(ec));
    try {
        std::lock_guard<std::mutex> lk(e->mu);
        struct OffAtExit { Scanner& s; ~OffAtExit() { s.set_extract_text(-1); } } off{*e->scanner};   // extract_chunk stays what it is
        e->scanner->set_extract_text((int)format);
        if (getenv("MATCHY_AMD_TRACE")) e->scanner->set_profile(true);   // the trace line names the extraction kernels' time beside the pass's
        ScanOutput so;
        e->scanner->scan_host(data, len, false, true, so, nullptr, nullptr, nullptr, nullptr);
        const ExtractTextView& v = so.extract_text;
        out->status = v.status;
        if (v.status != XR_OK) return MATCHY_SUCCESS;
        out->text = v.text; out->text_len = v.len; out->n_records = v.n_records;
        for (int t = 0; t < IT_COUNT; ++t) out->by_type[t] = v.by_type[t];
        return MATCHY_SUCCESS;
    } catch (const HipError& ex) { set_error(ex.what); return MATCHY_ERROR_IO; }
    catch (const std::exception& ex) { set_error(ex.what()); return MATCHY_ERROR_IO; }
}
void matchy_amd_extractor_get_render_timing(const matchy_extractor_t* ec, float out[4]) {
    if (!out) return;
    for (int k = 0; k < 4; ++k) out[k] = 0;
    if (!ec) return;
    ExtractorH* e = const_cast<ExtractorH*>(reinterpret_cast<const ExtractorH*>(ec));
    std::lock_guard<std::mutex> lk(e->mu);
    e->scanner->extract_text_timing(out);
}
uint64_t matchy_amd_extractor_render_allocations(const matchy_extractor_t* ec) {
    if (!ec) return 0;
    ExtractorH* e = const_cast<ExtractorH*>(reinterpret_cast<const ExtractorH*>(ec));
    std::lock_guard<std::mutex> lk(e->mu);
    return e->scanner->extract_text_allocations();
}
void matchy_matches_free(matchy_matches_t* m) {
    if (!m) return;
    delete reinterpret_cast<MatchesInternal*>(m->_internal);
    m->items = nullptr; m->count = 0; m->_internal = nullptr;
}

// ------------------------------------------------------------------------------------------------ bulk scan
matchy_scanner_t* matchy_scanner_create(const matchy_t* dbc, uint32_t extract_flags, int32_t device) {
    if (!dbc || device < 0) return nullptr;
    Db* db = const_cast<Db*>(reinterpret_cast<const Db*>(dbc));
    try {
        if (extract_flags == 0) {  // match_cmd.rs:276-303
            if (db->img->has_ip) extract_flags |= EX_IPV4 | EX_IPV6;
            if (db->img->has_literal || db->img->has_glob) extract_flags |= EX_DOMAINS | EX_EMAILS | EX_HASHES | EX_BITCOIN | EX_ETHEREUM | EX_MONERO;
        }
        std::shared_ptr<DeviceDb> ddb;
        { std::lock_guard<std::mutex> lk(db->mu); ddb = db->device_db(device); }
        auto s = std::make_unique<ScannerH>();
        s->db = db;
        s->sc = std::make_unique<Scanner>(db->img, ddb, extract_flags, 2);
        return reinterpret_cast<matchy_scanner_t*>(s.release());
    } catch (const HipError& e) { set_error(e.what); return nullptr; }
    catch (const std::exception& e) { set_error(e.what()); return nullptr; }
}
void matchy_scanner_free(matchy_scanner_t* s) { delete reinterpret_cast<ScannerH*>(s); }
void matchy_scanner_set_profile(matchy_scanner_t* s, bool on) { if (s) reinterpret_cast<ScannerH*>(s)->sc->set_profile(on); }
void matchy_scanner_set_slices(matchy_scanner_t* s, int32_t n) { if (s) reinterpret_cast<ScannerH*>(s)->sc->set_slices(n); }
int32_t matchy_scanner_last_slices(const matchy_scanner_t* s) { return s ? reinterpret_cast<const ScannerH*>(s)->sc->last_slice_count() : 0; }
void matchy_scanner_set_line_context(matchy_scanner_t* s, bool on) { if (s) reinterpret_cast<ScannerH*>(s)->sc->set_line_context(on); }
bool matchy_scanner_line_context(const matchy_scanner_t* s) { return s && reinterpret_cast<const ScannerH*>(s)->sc->line_context(); }
void matchy_scanner_get_line_timing(const matchy_scanner_t* s, float out[3]) {
    if (s && out) reinterpret_cast<const ScannerH*>(s)->sc->line_timing(out);
}
int32_t matchy_scan_result_lines(const matchy_scan_result_t* r, const matchy_scan_line_t** lines, const matchy_scan_line_t** ip4_lines, uint64_t* lines_with_matches) {
    if (!r) return MATCHY_ERROR_INVALID_PARAM;
    const ScanResultInternal* in = reinterpret_cast<const ScanResultInternal*>(r->_internal);
    if (!in || !in->has_lines) { set_error("matchy_scan_result_lines: the result was produced with line context off"); return MATCHY_ERROR_INVALID_PARAM; }
    if (lines) *lines = in->lines;
    if (ip4_lines) *ip4_lines = in->ip4_lines;
    if (lines_with_matches) *lines_with_matches = in->lines_with_matches;
    return MATCHY_SUCCESS;
}

// hit lines (Scanner::set_hit_lines, hit_lines.hip)
void matchy_scanner_set_hit_lines(matchy_scanner_t* s, bool on) { if (s) reinterpret_cast<ScannerH*>(s)->sc->set_hit_lines(on); }
bool matchy_scanner_hit_lines(const matchy_scanner_t* s) { return s && reinterpret_cast<const ScannerH*>(s)->sc->hit_lines(); }
int32_t matchy_scan_result_hit_lines(const matchy_scan_result_t* r, matchy_scan_hit_lines_t* out) {
    if (!r || !out) return MATCHY_ERROR_INVALID_PARAM;
    const ScanResultInternal* in = reinterpret_cast<const ScanResultInternal*>(r->_internal);
    if (!in || !in->has_hit_lines) { set_error("matchy_scan_result_hit_lines: the result was produced with hit lines off"); return MATCHY_ERROR_INVALID_PARAM; }
    *out = in->hit_lines;
    return MATCHY_SUCCESS;
}
void matchy_scanner_get_hit_lines_timing(const matchy_scanner_t* s, float out[3]) {
    if (s && out) reinterpret_cast<const ScannerH*>(s)->sc->hit_lines_timing(out);
}

// whole-line queries (Scanner::set_whole_lines, whole_lines.hip)
void matchy_scanner_set_whole_lines(matchy_scanner_t* s, bool on) { if (s) reinterpret_cast<ScannerH*>(s)->sc->set_whole_lines(on); }
bool matchy_scanner_whole_lines(const matchy_scanner_t* s) { return s && reinterpret_cast<const ScannerH*>(s)->sc->whole_lines(); }
void matchy_scanner_get_whole_lines_counters(const matchy_scanner_t* s, uint64_t out[4]) {
    if (s && out) reinterpret_cast<const ScannerH*>(s)->sc->whole_lines_counters(out);
}
void matchy_scanner_get_whole_lines_timing(const matchy_scanner_t* s, float out[3]) {
    if (s && out) reinterpret_cast<const ScannerH*>(s)->sc->whole_lines_timing(out);
}

// segmented scans (Scanner::set_segments, segments.hip)
int32_t matchy_scanner_set_segments(matchy_scanner_t* s, const uint32_t* starts, size_t n) {
    if (!s) return MATCHY_ERROR_INVALID_PARAM;
    try { reinterpret_cast<ScannerH*>(s)->sc->set_segments(starts, n); return MATCHY_SUCCESS; }
    catch (const std::exception& e) { set_error(e.what()); return MATCHY_ERROR_OUT_OF_MEMORY; }
}
int32_t matchy_scan_result_segments(const matchy_scan_result_t* r, const uint32_t** segment_of_hit, const uint32_t** segment_of_ip4_hit,
                                    const matchy_scan_segment_t** segments, size_t* n_segments) {
    if (!r) return MATCHY_ERROR_INVALID_PARAM;
    const ScanResultInternal* in = reinterpret_cast<const ScanResultInternal*>(r->_internal);
    if (!in || !in->has_segments) { set_error("matchy_scan_result_segments: the result was produced by a scan without segments"); return MATCHY_ERROR_INVALID_PARAM; }
    if (segment_of_hit) *segment_of_hit = in->segment_of_hit;
    if (segment_of_ip4_hit) *segment_of_ip4_hit = in->segment_of_ip4_hit;
    if (segments) *segments = in->segments.data();
    if (n_segments) *n_segments = in->segments.size();
    return MATCHY_SUCCESS;
}

void matchy_scanner_get_segment_timing(const matchy_scanner_t* s, float out[3]) {
    if (s && out) reinterpret_cast<const ScannerH*>(s)->sc->segment_timing(out);
}

// hit tally (Scanner::set_tally, tally.hip): the table is the scanner's
void matchy_scanner_set_tally(matchy_scanner_t* s, bool on) {
    if (!s) return;
    try { reinterpret_cast<ScannerH*>(s)->sc->set_tally(on); } catch (const HipError& e) { set_error(e.what); }
}
bool matchy_scanner_tally(const matchy_scanner_t* s) { return s && reinterpret_cast<const ScannerH*>(s)->sc->tally(); }
void matchy_scanner_reset_tally(matchy_scanner_t* s) {
    if (!s) return;
    try { reinterpret_cast<ScannerH*>(s)->sc->reset_tally(); } catch (const HipError& e) { set_error(e.what); }
}
int32_t matchy_scanner_tally_top(matchy_scanner_t* s, size_t limit, matchy_tally_t* out) {
    if (!s || !out) return MATCHY_ERROR_INVALID_PARAM;
    memset(out, 0, sizeof(*out));
    try {
        std::vector<TallyEntry> rows;
        uint64_t distinct = 0, matches = 0;
        if (!scanner_tally_top(s, limit, rows, distinct, matches)) { set_error("matchy_scanner_tally_top: the tally was never enabled on this scanner"); return MATCHY_ERROR_INVALID_PARAM; }
        fill_tally(std::move(rows), distinct, matches, out);
        return MATCHY_SUCCESS;
    } catch (const HipError& e) { set_error(e.what); return MATCHY_ERROR_IO; }
    catch (const std::exception& e) { set_error(e.what()); return MATCHY_ERROR_IO; }
}
void matchy_tally_free(matchy_tally_t* t) {
    if (!t) return;
    delete reinterpret_cast<TallyInternal*>(t->_internal);
    memset(t, 0, sizeof(*t));
}

void matchy_scanner_get_timing(const matchy_scanner_t* s, float out[5]) {
    if (!s || !out) return;
    const ScanTiming& t = reinterpret_cast<const ScannerH*>(s)->sc->timing();
    out[0] = t.anchor_ms; out[1] = t.validate_ms; out[2] = t.rare_ms; out[3] = t.lookup_ms; out[4] = t.total_ms;
}

int32_t matchy_scanner_scan(matchy_scanner_t* s, const uint8_t* data, size_t len, matchy_scan_result_t* out) {
    if (!s || !out || (!data && len) || len > 0xFFFFFFFFull) return MATCHY_ERROR_INVALID_PARAM;
    ScannerH* h = reinterpret_cast<ScannerH*>(s);
    try {
        ScanOutput so;
        std::vector<FinalHit> fin;
        std::vector<uint32_t> fids;
        std::vector<long long> foffs;
        std::vector<LineRec> flines;
        h->sc->scan_host(data, len, true, false, so, nullptr, &fin, &fids, &foffs, &flines);
        fill_result(fin.data(), fin.size(), fids.data(), foffs.data(), fids.size(), so.lines, so.n_cand, len, false, out);
        so.fin_lines = flines.data(); so.n_fin = flines.size();   // the merged line records, where an owned result copies them from
        attach_lines(*h->sc, so, Placement::OWNED, out);
        attach_segments(*h->sc, so, Placement::OWNED, out);
        attach_render(so, Placement::OWNED, out);   // scan_host put the pieces' blocks end to end: the result takes a copy
        // The one attachment that differs from attach_hit_lines: scan_host merged the pieces' blocks into vectors of its own, and the
        // result takes them by move instead of copying out of a pinned block.
        if (h->sc->hit_lines()) {
            auto* in = reinterpret_cast<ScanResultInternal*>(out->_internal);
            in->has_hit_lines = true;
            in->hl_text_own.swap(so.hl_text_own);
            in->hl_index_own = std::move(so.hl_off_own);
            if (in->hl_index_own.empty()) in->hl_index_own.push_back(0);
            const size_t n_lines = so.hl_no_own.size(), n_of = so.hl_of_own.size();
            in->hl_index_own.insert(in->hl_index_own.end(), so.hl_no_own.begin(), so.hl_no_own.end());
            in->hl_index_own.insert(in->hl_index_own.end(), so.hl_of_own.begin(), so.hl_of_own.end());
            const uint32_t* w = in->hl_index_own.data();
            matchy_scan_hit_lines_t& hl = in->hit_lines;
            hl = matchy_scan_hit_lines_t{};
            hl.text = in->hl_text_own.empty() ? nullptr : in->hl_text_own.data(); hl.text_len = in->hl_text_own.size(); hl.n_lines = (uint32_t)n_lines;
            hl.line_off = w; hl.line_no = n_lines ? w + n_lines + 1 : nullptr; hl.line_of_hit = n_of ? w + 2 * n_lines + 1 : nullptr;
        }
        return MATCHY_SUCCESS;
    } catch (const ParamError& e) { set_error(e.what); memset(out, 0, sizeof(*out)); return MATCHY_ERROR_INVALID_PARAM; }   // thrown in front of fill_result
    catch (const HipError& e) { set_error(e.what); return MATCHY_ERROR_IO; }
    catch (const std::exception& e) { set_error(e.what()); return MATCHY_ERROR_IO; }
}

int32_t matchy_scanner_scan_device(matchy_scanner_t* s, const void* dptr, size_t len, void* stream, uint32_t fetch_mode, matchy_scan_result_t* out) {
    if (!s || !out || !dptr) return MATCHY_ERROR_INVALID_PARAM;
    if (len >= 0x7FFF0000ull) return MATCHY_ERROR_INVALID_PARAM;
    ScannerH* h = reinterpret_cast<ScannerH*>(s);
    try {
        hipStream_t st = reinterpret_cast<hipStream_t>(stream);
        const FetchPlan plan(fetch_mode);
        ScanRequest rq;
        const bool hit_lines = build_request(*h->sc, plan, reinterpret_cast<const uint8_t*>(dptr), len, st, true, false, rq);
        h->sc->scan_device(rq, st);
        ScanOutput so;
        h->sc->fetch(so, false, st, plan.hit_mode(), plan.sorted);
        finish_result(*h->sc, plan, so, len, hit_lines, out);
        return MATCHY_SUCCESS;
    } catch (const ParamError& e) { set_error(e.what); memset(out, 0, sizeof(*out)); return MATCHY_ERROR_INVALID_PARAM; }   // thrown in front of fill_result
    catch (const HipError& e) { set_error(e.what); return MATCHY_ERROR_IO; }
    catch (const std::exception& e) { set_error(e.what()); return MATCHY_ERROR_IO; }
}

// The two halves of matchy_scanner_scan_device: submit launches the kernels of one batch on `stream` and returns; wait
// blocks until that batch is done and hands out its result. A host that keeps two scanners busy (each on its own stream)
// overlaps one batch's result transfer and latency-bound kernels with the next batch's streaming kernel.
int32_t matchy_scanner_submit_device(matchy_scanner_t* s, const void* dptr, size_t len, void* stream, uint32_t fetch_mode) {
    if (!s || !dptr) return MATCHY_ERROR_INVALID_PARAM;
    if (len >= 0x7FFF0000ull) return MATCHY_ERROR_INVALID_PARAM;
    ScannerH* h = reinterpret_cast<ScannerH*>(s);
    try {
        hipStream_t st = reinterpret_cast<hipStream_t>(stream);
        ScanRequest rq;   // not forked: several batches in flight (ScanRequest::fork)
        h->pending_hit_lines = build_request(*h->sc, FetchPlan(fetch_mode), reinterpret_cast<const uint8_t*>(dptr), len, st, false, false, rq);
        h->sc->scan_device(rq, st);
        h->pending = true; h->pending_len = len; h->pending_mode = fetch_mode; h->pending_stream = stream;
        return MATCHY_SUCCESS;
    } catch (const ParamError& e) { set_error(e.what); return MATCHY_ERROR_INVALID_PARAM; }
    catch (const HipError& e) { set_error(e.what); return MATCHY_ERROR_IO; }
    catch (const std::exception& e) { set_error(e.what()); return MATCHY_ERROR_IO; }
}
int32_t matchy_scanner_wait(matchy_scanner_t* s, matchy_scan_result_t* out) {
    if (!s || !out) return MATCHY_ERROR_INVALID_PARAM;
    ScannerH* h = reinterpret_cast<ScannerH*>(s);
    if (!h->pending) { set_error("matchy_scanner_wait: nothing was submitted"); return MATCHY_ERROR_INVALID_PARAM; }
    h->pending = false;
    try {
        const FetchPlan plan(h->pending_mode);
        ScanOutput so;
        h->sc->fetch(so, false, reinterpret_cast<hipStream_t>(h->pending_stream), plan.hit_mode(), plan.sorted);
        finish_result(*h->sc, plan, so, h->pending_len, h->pending_hit_lines, out);
        return MATCHY_SUCCESS;
    } catch (const ParamError& e) { set_error(e.what); memset(out, 0, sizeof(*out)); return MATCHY_ERROR_INVALID_PARAM; }   // thrown in front of fill_result
    catch (const HipError& e) { set_error(e.what); return MATCHY_ERROR_IO; }
    catch (const std::exception& e) { set_error(e.what()); return MATCHY_ERROR_IO; }
}

// gz scans (Scanner::gz_inflate, inflate.hip): inflate, seal, segment table and scan are queued on the scanner's own stream; the fetch is
// that of matchy_scanner_scan_device
static_assert(sizeof(GzMemberIn) == sizeof(matchy_gz_member_t) && offsetof(GzMemberIn, out_len) == offsetof(matchy_gz_member_t, out_len), "the plan reads matchy_gz_member_t directly");
static_assert(MATCHY_GZ_OK == gz::GZ_OK && MATCHY_GZ_BAD_HEADER == gz::GZ_BAD_HEADER && MATCHY_GZ_TRUNCATED == gz::GZ_TRUNCATED && MATCHY_GZ_BAD_BLOCK == gz::GZ_BAD_BLOCK &&
                  MATCHY_GZ_BAD_CODES == gz::GZ_BAD_CODES && MATCHY_GZ_BAD_SYMBOL == gz::GZ_BAD_SYMBOL && MATCHY_GZ_BAD_DISTANCE == gz::GZ_BAD_DISTANCE &&
                  MATCHY_GZ_OVERFLOW == gz::GZ_OVERFLOW && MATCHY_GZ_SIZE_MISMATCH == gz::GZ_SIZE_MISMATCH && MATCHY_GZ_CRC_MISMATCH == gz::GZ_CRC_MISMATCH &&
                  MATCHY_GZ_TRAILING_DATA == gz::GZ_TRAILING_DATA, "k_gz_inflate writes MATCHY_GZ_* values directly");
static_assert(sizeof(GzFileIn) == sizeof(matchy_gz_file_t) && offsetof(GzFileIn, len) == offsetof(matchy_gz_file_t, len), "the plan reads matchy_gz_file_t directly");
// one table is set: `members` (matchy_scanner_scan_gz: one member per file, member i is segment i) or `files` (matchy_scanner_scan_gz_files:
// files of one member or many, file i is segment i), or `window` (matchy_scanner_scan_gz_window: packed[0, packed_len) are the whole members of
// one window, which is segment 0)
static int32_t scan_gz_pack(ScannerH* h, const uint8_t* packed, size_t packed_len, const matchy_gz_member_t* members, const matchy_gz_file_t* files, size_t n,
                            uint32_t fetch_mode, bool want_text, matchy_scan_result_t* out, const matchy_gz_window_t* window = nullptr,
                            const matchy_gz_stream_window_t* sw = nullptr) {
    try {
        { ScanRequest mode; mode.lookup = true; h->sc->arm_whole_lines(mode, true); }   // refused in front of the inflate kernels
        const Scanner::GzBatch b = sw ? h->sc->gz_inflate_stream(packed, packed_len, reinterpret_cast<const gz::StreamState*>(sw->state), sw->carry, sw->carry_len, sw->carry_cap,
                                                                  sw->text_cap, (sw->flags & MATCHY_STREAM_FIRST) != 0, (sw->flags & MATCHY_STREAM_FILE_END) != 0)
                                   : window ? h->sc->gz_inflate_window(packed, packed_len, window->carry, window->carry_len, window->carry_cap, (window->flags & MATCHY_WINDOW_LAST) != 0)
                                   : files ? h->sc->gz_inflate_files(packed, packed_len, reinterpret_cast<const GzFileIn*>(files), n)
                                           : h->sc->gz_inflate(packed, packed_len, reinterpret_cast<const GzMemberIn*>(members), n);
        const FetchPlan plan(fetch_mode);
        ScanRequest rq;   // not forked: the scan shares the stream of the pass in front of it
        const bool hit_lines = build_request(*h->sc, plan, b.text, b.len, b.stream, false, true, rq);
        h->sc->scan_device(rq, b.stream);
        h->sc->gz_queue_results(want_text);
        ScanOutput so;
        h->sc->fetch(so, false, b.stream, plan.hit_mode(), plan.sorted);
        const GzInflate::Result g = h->sc->gz_finish();
        finish_result(*h->sc, plan, so, g.ok_bytes, hit_lines, out);
        out->lines = so.lines - std::min<uint64_t>(so.lines, g.not_input_nl);
        ScanResultInternal* in = internal_of(out);
        in->has_gz = true;
        in->gz_status.assign(g.status, g.status + g.n);
        if (g.file_status) {
            in->has_gz_files = true;
            in->gz_file_status.assign(g.file_status, g.file_status + g.n_files);
            in->gz_first_member.assign(g.first_member, g.first_member + g.n_files + 1);
        }
        in->gz_text = g.text; in->gz_text_len = g.text_len;
        if (plan.sorted && g.text) { in->gz_text_own.assign(g.text, g.text + g.text_len); in->gz_text = in->gz_text_own.data(); }
        if (g.first_piece) {   // pieces are on: the table may still be empty
            in->has_gz_pieces = true;
            in->gz_first_piece.assign(g.first_piece, g.first_piece + g.n + 1);
            in->gz_pieces.resize(g.n_pieces);
            for (size_t k = 0; k < g.n_pieces; ++k) memcpy(&in->gz_pieces[k], &g.pieces[k], sizeof(matchy_gz_piece_t));
        }
        if (g.window) {   // the carry is the next window's input while this result may already be freed by then: always owned
            in->has_gz_window = true;
            in->gz_window_status = g.window_status;
            in->gz_carry.assign(g.carry, g.carry + g.carry_len);
        }
        if (g.stream) {   // state and carry are the next window's input: always owned
            in->has_gz_stream = true;
            in->gz_stream_status = g.stream_status; in->gz_stream_gz_status = g.stream_gz_status;
            in->gz_stream_consumed_bits = g.consumed_bits; in->gz_stream_text_len = g.stream_text_len; in->gz_stream_ended = g.ended;
            if (g.state_out) { in->gz_stream_state.resize(1); memcpy(in->gz_stream_state.data(), g.state_out, sizeof(matchy_gz_stream_state_t)); }
            if (g.carry_len) in->gz_carry.assign(g.carry, g.carry + g.carry_len);
        }
        return MATCHY_SUCCESS;
    } catch (const ParamError& e) { set_error(e.what); matchy_scan_result_free(out); return MATCHY_ERROR_INVALID_PARAM; }
    catch (const HipError& e) { set_error(e.what); return MATCHY_ERROR_IO; }
    catch (const std::exception& e) { set_error(e.what()); return MATCHY_ERROR_IO; }
}
// UTF-16 inputs (Scanner::utf16_transcode, utf16.hip): scan_front_text does the scan behind the pass
static_assert(MATCHY_UTF16_LE == utf16::ORDER_LE && MATCHY_UTF16_BE == utf16::ORDER_BE, "the kernels take MATCHY_UTF16_* values directly");
int32_t matchy_scanner_scan_utf16(matchy_scanner_t* s, const uint8_t* data, size_t len, uint32_t byte_order, uint32_t fetch_mode, bool want_text, matchy_scan_result_t* out) {
    if (!s || !out) { set_error("matchy_scanner_scan_utf16: no scanner or no result"); return MATCHY_ERROR_INVALID_PARAM; }
    memset(out, 0, sizeof(*out));
    if (const char* why = utf16_refusal(data, len, byte_order)) { set_error(std::string("matchy_scanner_scan_utf16: ") + why); return MATCHY_ERROR_INVALID_PARAM; }
    ScannerH* h = reinterpret_cast<ScannerH*>(s);
    try {
        const Scanner::GzBatch b = h->sc->utf16_transcode(data, len, byte_order);   // refuses segments and whole-line mode
        const Utf16Transcode::Result u = scan_front_text(h, b, fetch_mode, "matchy_scanner_scan_utf16", [&] { h->sc->utf16_queue_text(want_text); },
                                                         [&] { return h->sc->utf16_finish(); }, out);
        ScanResultInternal* in = internal_of(out);
        in->has_utf16 = true;
        in->utf16_code_units = u.code_units; in->utf16_replaced = u.replaced;
        return MATCHY_SUCCESS;
    } catch (const ParamError& e) { set_error(e.what); matchy_scan_result_free(out); return MATCHY_ERROR_INVALID_PARAM; }
    catch (const HipError& e) { set_error(e.what); return MATCHY_ERROR_IO; }
    catch (const std::exception& e) { set_error(e.what()); return MATCHY_ERROR_IO; }
}
int32_t matchy_scan_result_utf16(const matchy_scan_result_t* r, const uint8_t** text, size_t* text_len, uint64_t* code_units, uint64_t* replaced) {
    if (!r) { set_error("matchy_scan_result_utf16: no result"); return MATCHY_ERROR_INVALID_PARAM; }
    const ScanResultInternal* in = reinterpret_cast<const ScanResultInternal*>(r->_internal);
    if (!in || !in->has_utf16) { set_error("matchy_scan_result_utf16: the result was not produced by a UTF-16 scan"); return MATCHY_ERROR_INVALID_PARAM; }
    if (text) *text = in->front_text;
    if (text_len) *text_len = in->front_text_len;
    if (code_units) *code_units = in->utf16_code_units;
    if (replaced) *replaced = in->utf16_replaced;
    return MATCHY_SUCCESS;
}
void matchy_scanner_get_utf16_timing(const matchy_scanner_t* s, float out[3]) {
    if (s && out) reinterpret_cast<const ScannerH*>(s)->sc->utf16_timing(out);
}
void matchy_amd_utf16_geometry(uint32_t out[2]) {
    if (out) { out[0] = utf16::TILE_BYTES; out[1] = UTF16_SCAN_CHUNK; }
}

// Percent- and JSON-escaped inputs (Scanner::unescape, unescape.hip)
static_assert(MATCHY_UNESCAPE_PERCENT == unescape::MODE_PERCENT && MATCHY_UNESCAPE_JSON == unescape::MODE_JSON, "the pass takes MATCHY_UNESCAPE_* values directly");
int32_t matchy_scanner_scan_escaped(matchy_scanner_t* s, const uint8_t* data, size_t len, uint32_t modes, uint32_t fetch_mode, bool want_text, matchy_scan_result_t* out) {
    if (!s || !out) { set_error("matchy_scanner_scan_escaped: no scanner or no result"); return MATCHY_ERROR_INVALID_PARAM; }
    memset(out, 0, sizeof(*out));
    if (const char* why = unescape_refusal(data, len, modes)) { set_error(std::string("matchy_scanner_scan_escaped: ") + why); return MATCHY_ERROR_INVALID_PARAM; }
    ScannerH* h = reinterpret_cast<ScannerH*>(s);
    try {
        const Scanner::GzBatch b = h->sc->unescape(data, len, modes);   // refuses segments and whole-line mode
        const Unescape::Result u = scan_front_text(h, b, fetch_mode, "matchy_scanner_scan_escaped", [&] { h->sc->unescape_queue_text(want_text); },
                                                   [&] { return h->sc->unescape_finish(); }, out);
        ScanResultInternal* in = internal_of(out);
        in->has_unescaped = true;
        in->unescape_counters[0] = u.escapes; in->unescape_counters[1] = u.replaced; in->unescape_counters[2] = u.lf_escapes;
        return MATCHY_SUCCESS;
    } catch (const ParamError& e) { set_error(e.what); matchy_scan_result_free(out); return MATCHY_ERROR_INVALID_PARAM; }
    catch (const HipError& e) { set_error(e.what); return MATCHY_ERROR_IO; }
    catch (const std::exception& e) { set_error(e.what()); return MATCHY_ERROR_IO; }
}
int32_t matchy_scan_result_unescaped(const matchy_scan_result_t* r, const uint8_t** text, size_t* text_len, uint64_t counters[3]) {
    if (!r) { set_error("matchy_scan_result_unescaped: no result"); return MATCHY_ERROR_INVALID_PARAM; }
    const ScanResultInternal* in = reinterpret_cast<const ScanResultInternal*>(r->_internal);
    if (!in || !in->has_unescaped) { set_error("matchy_scan_result_unescaped: the result was not produced by an escaped scan"); return MATCHY_ERROR_INVALID_PARAM; }
    if (text) *text = in->front_text;
    if (text_len) *text_len = in->front_text_len;
    if (counters) for (int k = 0; k < 3; ++k) counters[k] = in->unescape_counters[k];
    return MATCHY_SUCCESS;
}
void matchy_scanner_get_unescape_timing(const matchy_scanner_t* s, float out[3]) {
    if (s && out) reinterpret_cast<const ScannerH*>(s)->sc->unescape_timing(out);
}
void matchy_amd_unescape_geometry(uint32_t out[3]) {
    if (out) { out[0] = unescape::TILE_BYTES; out[1] = UNESCAPE_SCAN_CHUNK; out[2] = UNESCAPE_STATE_CHUNK; }
}

int32_t matchy_scanner_scan_gz(matchy_scanner_t* s, const uint8_t* packed, size_t packed_len, const matchy_gz_member_t* members, size_t n, uint32_t fetch_mode,
                               bool want_text, matchy_scan_result_t* out) {
    if (!s || !out) return MATCHY_ERROR_INVALID_PARAM;
    memset(out, 0, sizeof(*out));
    if (!members || n == 0 || (!packed && packed_len)) { set_error("matchy_scanner_scan_gz: no members"); return MATCHY_ERROR_INVALID_PARAM; }
    return scan_gz_pack(reinterpret_cast<ScannerH*>(s), packed, packed_len, members, nullptr, n, fetch_mode, want_text, out);
}
int32_t matchy_scanner_scan_gz_files(matchy_scanner_t* s, const uint8_t* packed, size_t packed_len, const matchy_gz_file_t* files, size_t n_files, uint32_t fetch_mode,
                                     bool want_text, matchy_scan_result_t* out) {
    if (!s || !out) return MATCHY_ERROR_INVALID_PARAM;
    memset(out, 0, sizeof(*out));
    if (!files || n_files == 0 || (!packed && packed_len)) { set_error("matchy_scanner_scan_gz_files: no files"); return MATCHY_ERROR_INVALID_PARAM; }
    return scan_gz_pack(reinterpret_cast<ScannerH*>(s), packed, packed_len, nullptr, files, n_files, fetch_mode, want_text, out);
}
static_assert(MATCHY_WINDOW_OK == GZ_WINDOW_OK && MATCHY_WINDOW_NO_LINE_END == GZ_WINDOW_NO_LINE_END, "k_gz_window_tail writes MATCHY_WINDOW_* values directly");
int32_t matchy_scanner_scan_gz_window(matchy_scanner_t* s, const uint8_t* packed, size_t packed_len, const matchy_gz_window_t* window, uint32_t fetch_mode, bool want_text,
                                      matchy_scan_result_t* out) {
    if (!s || !out) { set_error("matchy_scanner_scan_gz_window: no scanner or no result"); return MATCHY_ERROR_INVALID_PARAM; }
    memset(out, 0, sizeof(*out));
    if (const char* why = gz_window_refusal(packed, packed_len, window)) { set_error(std::string("matchy_scanner_scan_gz_window: ") + why); return MATCHY_ERROR_INVALID_PARAM; }
    return scan_gz_pack(reinterpret_cast<ScannerH*>(s), packed, packed_len, nullptr, nullptr, 1, fetch_mode, want_text, out, window);
}
static_assert(sizeof(matchy_gz_stream_state_t) == sizeof(gz::StreamState) && offsetof(matchy_gz_stream_state_t, history) == offsetof(gz::StreamState, history) &&
                  offsetof(matchy_gz_stream_state_t, bit) == offsetof(gz::StreamState, bit), "the pass reads matchy_gz_stream_state_t directly");
static_assert(MATCHY_STREAM_OK == gz::STREAM_OK && MATCHY_STREAM_NO_LINE_END == gz::STREAM_NO_LINE_END && MATCHY_STREAM_NO_PROGRESS == gz::STREAM_NO_PROGRESS &&
                  MATCHY_STREAM_FAILED == gz::STREAM_FAILED && MATCHY_STREAM_FIRST == GZ_STREAM_FIRST && MATCHY_STREAM_FILE_END == GZ_STREAM_FILE_END &&
                  MATCHY_STREAM_PASSES == GZ_STREAM_PASSES, "k_gz_stream_verdict writes MATCHY_STREAM_* values directly");
int32_t matchy_scanner_scan_gz_stream(matchy_scanner_t* s, const uint8_t* packed, size_t packed_len, const matchy_gz_stream_window_t* window, uint32_t fetch_mode, bool want_text,
                                      matchy_scan_result_t* out) {
    if (!s || !out) { set_error("matchy_scanner_scan_gz_stream: no scanner or no result"); return MATCHY_ERROR_INVALID_PARAM; }
    memset(out, 0, sizeof(*out));
    if (const char* why = gz_stream_refusal(packed, packed_len, window)) { set_error(std::string("matchy_scanner_scan_gz_stream: ") + why); return MATCHY_ERROR_INVALID_PARAM; }
    if (!reinterpret_cast<ScannerH*>(s)->sc->gz_pieces()) { set_error("matchy_scanner_scan_gz_stream: pieces of one stream are off (matchy_scanner_set_gz_pieces comes first)"); return MATCHY_ERROR_INVALID_PARAM; }
    return scan_gz_pack(reinterpret_cast<ScannerH*>(s), packed, packed_len, nullptr, nullptr, 1, fetch_mode, want_text, out, nullptr, window);
}
int32_t matchy_scan_result_gz_stream(const matchy_scan_result_t* r, int32_t* status, int32_t* gz_status, uint64_t* consumed_bits, uint32_t* text_len, bool* ended,
                                     const matchy_gz_stream_state_t** state_out, const uint8_t** carry, size_t* carry_len) {
    if (!r) { set_error("matchy_scan_result_gz_stream: no result"); return MATCHY_ERROR_INVALID_PARAM; }
    const ScanResultInternal* in = reinterpret_cast<const ScanResultInternal*>(r->_internal);
    if (!in || !in->has_gz_stream) { set_error("matchy_scan_result_gz_stream: the result was not produced by a gz scan of a stream window"); return MATCHY_ERROR_INVALID_PARAM; }
    if (status) *status = in->gz_stream_status;
    if (gz_status) *gz_status = in->gz_stream_gz_status;
    if (consumed_bits) *consumed_bits = in->gz_stream_consumed_bits;
    if (text_len) *text_len = in->gz_stream_text_len;
    if (ended) *ended = in->gz_stream_ended;
    if (state_out) *state_out = in->gz_stream_state.empty() ? nullptr : in->gz_stream_state.data();
    if (carry) *carry = in->gz_carry.data();
    if (carry_len) *carry_len = in->gz_carry.size();
    return MATCHY_SUCCESS;
}
void matchy_scanner_get_gz_stream_timing(const matchy_scanner_t* s, float out[MATCHY_STREAM_PASSES]) {
    if (s && out) reinterpret_cast<const ScannerH*>(s)->sc->gz_stream_timing(out);
}
int32_t matchy_scan_result_gz_window(const matchy_scan_result_t* r, int32_t* window_status, const uint8_t** carry, size_t* carry_len) {
    if (!r) { set_error("matchy_scan_result_gz_window: no result"); return MATCHY_ERROR_INVALID_PARAM; }
    const ScanResultInternal* in = reinterpret_cast<const ScanResultInternal*>(r->_internal);
    if (!in || !in->has_gz_window) { set_error("matchy_scan_result_gz_window: the result was not produced by a gz scan of a window"); return MATCHY_ERROR_INVALID_PARAM; }
    if (window_status) *window_status = in->gz_window_status;
    if (carry) *carry = in->gz_carry.data();
    if (carry_len) *carry_len = in->gz_carry.size();
    return MATCHY_SUCCESS;
}
void matchy_scanner_get_gz_window_timing(const matchy_scanner_t* s, float out[4]) {
    if (s && out) reinterpret_cast<const ScannerH*>(s)->sc->gz_window_timing(out);
}
int32_t matchy_scan_result_gz_files(const matchy_scan_result_t* r, const int32_t** file_status, size_t* n_files, const uint32_t** first_member) {
    if (!r) return MATCHY_ERROR_INVALID_PARAM;
    const ScanResultInternal* in = reinterpret_cast<const ScanResultInternal*>(r->_internal);
    if (!in || !in->has_gz_files) { set_error("matchy_scan_result_gz_files: the result was not produced by a gz scan of files"); return MATCHY_ERROR_INVALID_PARAM; }
    if (file_status) *file_status = in->gz_file_status.data();
    if (n_files) *n_files = in->gz_file_status.size();
    if (first_member) *first_member = in->gz_first_member.data();
    return MATCHY_SUCCESS;
}
int32_t matchy_scan_result_gz(const matchy_scan_result_t* r, const int32_t** status, size_t* n_members, const uint8_t** text, size_t* text_len) {
    if (!r) return MATCHY_ERROR_INVALID_PARAM;
    const ScanResultInternal* in = reinterpret_cast<const ScanResultInternal*>(r->_internal);
    if (!in || !in->has_gz) { set_error("matchy_scan_result_gz: the result was not produced by a gz scan"); return MATCHY_ERROR_INVALID_PARAM; }
    if (status) *status = in->gz_status.data();
    if (n_members) *n_members = in->gz_status.size();
    if (text) *text = in->gz_text;
    if (text_len) *text_len = in->gz_text_len;
    return MATCHY_SUCCESS;
}
static_assert(sizeof(matchy_gz_piece_t) == 32 && offsetof(matchy_gz_piece_t, flags) == offsetof(gz::Piece, flags) && offsetof(matchy_gz_piece_t, member) == offsetof(gz::Piece, member),
              "matchy_gz_piece_t is the first 32 bytes of gz::Piece");
static_assert(MATCHY_PIECE_HAS_START == gz::PIECE_HAS_START && MATCHY_PIECE_LIVE == gz::PIECE_LIVE && MATCHY_PIECE_HANDED_OVER == gz::PIECE_HANDED, "the kernels write MATCHY_PIECE_* flags directly");
int32_t matchy_scanner_set_gz_pieces(matchy_scanner_t* s, uint32_t piece_bytes) {
    if (!s) { set_error("matchy_scanner_set_gz_pieces: no scanner"); return MATCHY_ERROR_INVALID_PARAM; }
    if (piece_bytes && !gz_piece_bytes_valid(piece_bytes)) { set_error("matchy_scanner_set_gz_pieces: piece_bytes is 0 or a power of two from 512 to 1 MiB"); return MATCHY_ERROR_INVALID_PARAM; }
    reinterpret_cast<ScannerH*>(s)->sc->set_gz_pieces(piece_bytes);
    return MATCHY_SUCCESS;
}
uint32_t matchy_scanner_get_gz_pieces(const matchy_scanner_t* s) { return s ? reinterpret_cast<const ScannerH*>(s)->sc->gz_pieces() : 0; }
int32_t matchy_scan_result_gz_pieces(const matchy_scan_result_t* r, const matchy_gz_piece_t** pieces, size_t* n, const uint32_t** first_piece) {
    if (!r) { set_error("matchy_scan_result_gz_pieces: no result"); return MATCHY_ERROR_INVALID_PARAM; }
    const ScanResultInternal* in = reinterpret_cast<const ScanResultInternal*>(r->_internal);
    if (!in || !in->has_gz) { set_error("matchy_scan_result_gz_pieces: the result was not produced by a gz scan"); return MATCHY_ERROR_INVALID_PARAM; }
    if (pieces) *pieces = in->gz_pieces.data();
    if (n) *n = in->gz_pieces.size();
    if (first_piece) *first_piece = in->has_gz_pieces ? in->gz_first_piece.data() : nullptr;
    return MATCHY_SUCCESS;
}
void matchy_scanner_get_gz_pieces_timing(const matchy_scanner_t* s, float out[6]) {
    if (s && out) reinterpret_cast<const ScannerH*>(s)->sc->gz_pieces_timing(out);
}
void matchy_scanner_get_gz_timing(const matchy_scanner_t* s, float out[3]) {
    if (s && out) reinterpret_cast<const ScannerH*>(s)->sc->gz_timing(out);
}

// rendered records (Scanner::set_render, render.hip)
static_assert(MATCHY_RENDER_LINE_NUMBERS == render::FLAG_LINE_NUMBERS && MATCHY_RENDER_INPUT_LINE == render::FLAG_INPUT_LINE, "the kernels read the flags directly");
static_assert(MATCHY_RENDER_OK == RENDER_OK && MATCHY_RENDER_TOO_LARGE == RENDER_TOO_LARGE, "the kernels write MATCHY_RENDER_* values directly");
static_assert(MATCHY_SCAN_IP4_DATA_BITS == 22, "render.hip expands compact records with this layout");
int32_t matchy_scanner_set_render(matchy_scanner_t* s, const matchy_render_params_t* p) {
    if (!s) return MATCHY_ERROR_INVALID_PARAM;
    Scanner& sc = *reinterpret_cast<ScannerH*>(s)->sc;
    if (!p) { sc.set_render(nullptr); return MATCHY_SUCCESS; }
    if (p->flags & ~(MATCHY_RENDER_LINE_NUMBERS | MATCHY_RENDER_INPUT_LINE)) { set_error("matchy_scanner_set_render: unknown flags"); return MATCHY_ERROR_INVALID_PARAM; }
    if (p->sources && !p->n_sources) { set_error("matchy_scanner_set_render: sources without n_sources"); return MATCHY_ERROR_INVALID_PARAM; }
    try {
        RenderParams rp;
        rp.flags = p->flags | ((p->flags & MATCHY_RENDER_INPUT_LINE) ? MATCHY_RENDER_LINE_NUMBERS : 0u);
        auto escaped = [](const char* src) { std::string o; json_escape(src ? src : "-", o); return o; };
        if (p->sources) {
            rp.per_segment = true;
            for (size_t k = 0; k < p->n_sources; ++k) { rp.sources.push_back(escaped(p->sources[k])); rp.line_bases.push_back(p->line_bases ? p->line_bases[k] : 0); }
        } else { rp.sources.push_back(escaped(p->source)); rp.line_bases.push_back(p->line_base); }
        sc.set_render(&rp);
        return MATCHY_SUCCESS;
    } catch (const std::exception& e) { set_error(e.what()); return MATCHY_ERROR_OUT_OF_MEMORY; }
}
int32_t matchy_scan_result_ndjson(const matchy_scan_result_t* r, const char** text, uint64_t* len, int32_t* status) {
    if (!r) return MATCHY_ERROR_INVALID_PARAM;
    const ScanResultInternal* in = reinterpret_cast<const ScanResultInternal*>(r->_internal);
    if (!in || !in->has_render) { set_error("matchy_scan_result_ndjson: the scan of this result was not armed with matchy_scanner_set_render"); return MATCHY_ERROR_INVALID_PARAM; }
    if (text) *text = reinterpret_cast<const char*>(in->render_text);
    if (len) *len = in->render_len;
    if (status) *status = in->render_status;
    return MATCHY_SUCCESS;
}
void matchy_scanner_get_render_timing(const matchy_scanner_t* s, float out[3]) {
    if (s && out) reinterpret_cast<const ScannerH*>(s)->sc->render_timing(out);
}
void matchy_scanner_get_render_counters(const matchy_scanner_t* s, uint64_t out[6]) {
    if (!s || !out) return;
    for (int k = 0; k < 6; ++k) out[k] = 0;
    if (const NdjsonRender::Events* ev = reinterpret_cast<const ScannerH*>(s)->sc->render_events()) { out[0] = ev->rounds; out[1] = ev->misses; out[2] = ev->payloads_added; out[3] = ev->copied; out[4] = ev->rehashes; out[5] = ev->pool_regrows; }
}

void matchy_scan_result_free(matchy_scan_result_t* r) {
    if (!r) return;
    delete reinterpret_cast<ScanResultInternal*>(r->_internal);
    memset(r, 0, sizeof(*r));
}

bool matchy_scan_result_on_device(const matchy_scan_result_t* r) {
    return r && r->_internal && reinterpret_cast<const ScanResultInternal*>(r->_internal)->on_device;
}

// ------------------------------------------------------------------------------------------------ NDJSON on the host (ndjson_host.h)
// The plain view of a result for the host renderer. A host-resident result with hit lines and line context carries the text of its
// records itself (the block); any other needs the batch.
static ndjson::ResultView view_of(const matchy_scan_result_t* r, const uint8_t* text) {
    ndjson::ResultView v;
    v.hits = r->hits; v.n_hits = r->n_hits; v.ip4_hits = r->ip4_hits; v.n_ip4_hits = r->n_ip4_hits; v.data_offsets = r->data_offsets; v.text = text;
    const ScanResultInternal* in = reinterpret_cast<const ScanResultInternal*>(r->_internal);
    if (!in) return v;
    if (in->has_lines) { v.lines = in->lines; v.ip4_lines = in->ip4_lines; }
    if (in->has_segments) { v.segment_of_hit = in->segment_of_hit; v.segment_of_ip4_hit = in->segment_of_ip4_hit; v.segments = in->segments.data(); v.n_segments = in->segments.size(); }
    if (in->has_hit_lines && !in->on_device && in->has_lines) v.block = &in->hit_lines;
    return v;
}
static ndjson::Payloads payloads_of(const matchy_scanner_t* s) { return {&payload_json, &reinterpret_cast<const ScannerH*>(s)->sc->image()}; }

char* matchy_scan_hit_to_json(const matchy_scanner_t* s, const matchy_scan_result_t* r, size_t i, const uint8_t* text, const char* source) {
    // i counts through hits, then through the compact IPv4 records of a MATCHY_SCAN_FETCH_COMPACT result
    if (!s || !r || i >= r->n_hits + r->n_ip4_hits) return nullptr;
    const bool in_hits = i < r->n_hits;
    if (in_hits ? !r->hits : !r->ip4_hits) return nullptr;
    if (matchy_scan_result_on_device(r)) { set_error("matchy_scan_hit_to_json: the records of this result are in device memory (MATCHY_SCAN_FETCH_DEVICE)"); return nullptr; }
    std::string o;
    if (!ndjson::Renderer::record(view_of(r, text), in_hits, in_hits ? i : i - r->n_hits, source, payloads_of(s), o)) return nullptr;
    return strdup(o.c_str());
}

// Every match of a result as NDJSON — the text matchy_scan_hit_to_json returns for each, with the line keys of `k` and '\n' behind every
// line — in ONE call and one allocation.
static int32_t result_to_ndjson(matchy_scanner_t* s, const matchy_scan_result_t* r, const uint8_t* text, const ndjson::Keys& k, char** out, size_t* out_len) {
    if (!s || !r || !out || !out_len) return MATCHY_ERROR_INVALID_PARAM;
    ndjson::ResultView v = view_of(r, text);
    // a result renders from its block (`text` may be NULL) unless the block holds lines without their text (a counts-only fetch)
    if (v.block && !v.block->text && v.block->n_lines) v.block = nullptr;
    if (!v.block && !text && (r->n_hits || r->n_ip4_hits)) return MATCHY_ERROR_INVALID_PARAM;
    if (k.sources && matchy_scan_result_segments(r, nullptr, nullptr, nullptr, nullptr) != MATCHY_SUCCESS) return MATCHY_ERROR_INVALID_PARAM;
    if (k.with_lines && matchy_scan_result_lines(r, nullptr, nullptr, nullptr) != MATCHY_SUCCESS) return MATCHY_ERROR_INVALID_PARAM;
    if (matchy_scan_result_on_device(r)) { set_error("matchy_scan_result_to_ndjson: the records of this result are in device memory (MATCHY_SCAN_FETCH_DEVICE)"); return MATCHY_ERROR_INVALID_PARAM; }
    std::string error;
    const int32_t rc = reinterpret_cast<ScannerH*>(s)->ndjson.render(v, k, payloads_of(s), out, out_len, error);
    if (rc != MATCHY_SUCCESS) set_error(error);
    return rc;
}

int32_t matchy_scan_result_to_ndjson(matchy_scanner_t* s, const matchy_scan_result_t* r, const uint8_t* text, const char* source, char** out, size_t* out_len) {
    return result_to_ndjson(s, r, text, ndjson::Keys{source, nullptr, false, false, 0, nullptr}, out, out_len);
}
int32_t matchy_scan_result_to_ndjson_lines(matchy_scanner_t* s, const matchy_scan_result_t* r, const uint8_t* text, const char* source, uint64_t line_base,
                                           bool with_input_line, char** out, size_t* out_len) {
    return result_to_ndjson(s, r, text, ndjson::Keys{source, nullptr, true, with_input_line, line_base, nullptr}, out, out_len);
}
int32_t matchy_scan_result_to_ndjson_segments(matchy_scanner_t* s, const matchy_scan_result_t* r, const uint8_t* text, const char* const* sources,
                                              const uint64_t* line_bases, bool with_input_line, char** out, size_t* out_len) {
    if (!sources) return MATCHY_ERROR_INVALID_PARAM;
    return result_to_ndjson(s, r, text, ndjson::Keys{nullptr, sources, line_bases != nullptr, with_input_line, 0, line_bases}, out, out_len);
}

}  // extern "C"
