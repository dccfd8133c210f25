// The multi-device scanner of libmatchy_amd.so (matchy_multi_scanner_*, and the NUMA entry points its workers use), built on the
// public matchy_scanner_* calls only.
//
// The reader -> per-device workers -> ordered gather of `matchy match` (reference: process_files_parallel,
// crates/matchy/src/processing/parallel.rs:494-505 and its workers :594-704) behind the C ABI: the host submits newline-aligned
// batches, one worker thread per device entry scans them with a scanner of its own (host-buffer entry: the batch is pinned for its copy,
// results come back in canonical order), and the host takes the results back IN SUBMISSION ORDER. No data-path collective: line blocks
// are independent (N4), the database is replicated per device, the counters are summed by the caller.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <thread>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include "batch_reader.h"
#include "capi_internal.h"
#include "engine.h"
#include "host_topology.h"

using namespace mxy;
using namespace mxy::capi;

namespace {
// matchy_multi_scanner_set_render: the caller's parameters, copied, until the worker that takes the batch arms its scanner with them
struct RenderSpec {
    uint32_t flags = 0;
    bool per_segment = false;
    std::vector<std::string> sources;   // one, or one per segment
    std::vector<uint64_t> line_bases;   // parallel to sources
    void arm(matchy_scanner_t* sc) const {
        matchy_render_params_t p{};
        p.flags = flags;
        std::vector<const char*> ptrs;
        for (const std::string& s : sources) ptrs.push_back(s.c_str());
        if (per_segment) { p.sources = ptrs.data(); p.n_sources = ptrs.size(); p.line_bases = line_bases.data(); }
        else { p.source = ptrs[0]; p.line_base = line_bases[0]; }
        (void)matchy_scanner_set_render(sc, &p);   // copies
    }
};
// what a batch is: set by the submit call that queued it (matchy_multi_scanner_submit / _submit_near, _submit_segments, _submit_gz,
// _submit_gz_files, _submit_gz_window, _submit_gz_stream, _submit_utf16, _submit_escaped, in this order), read by the worker that scans it
enum class JobKind { PLAIN, SEGMENTS, GZ_MEMBERS, GZ_FILES, GZ_WINDOW, GZ_STREAM, UTF16, ESCAPED };
struct MultiJob {
    JobKind kind;
    const uint8_t* data;                      // the caller's bytes: text, or (gz kinds) the compressed pack
    size_t len;
    void* tag;
    size_t seq = 0;                           // given out when the job is queued
    const void* pinned = nullptr;             // PLAIN, SEGMENTS: page range the caller pinned; the worker unpins it
    int32_t node = -1;                        // NUMA node the bytes live on, -1 = anywhere
    std::vector<uint32_t> starts;             // SEGMENTS: the segments of the batch
    std::vector<matchy_gz_member_t> gz;       // GZ_MEMBERS: a pack of gzip files of one member each
    std::vector<matchy_gz_file_t> gz_files;   // GZ_FILES: of files of one member or many
    std::vector<uint8_t> carry;               // GZ_WINDOW: the batch is one window of a large file behind this carry, copied at the submit
    uint32_t carry_cap = 0, window_flags = 0; // GZ_WINDOW
    std::unique_ptr<matchy_gz_stream_state_t> stream_state;   // GZ_STREAM: the state of the window (none for the first), copied at the submit like the carry
    uint32_t stream_text_cap = 0;             // GZ_STREAM (carry, carry_cap and window_flags as for GZ_WINDOW)
    bool gz_text = false;                     // gz kinds: the inflated text comes back with the result; UTF16: the UTF-8 text; ESCAPED: the decoded text
    uint32_t byte_order = 0;                  // UTF16
    uint32_t unescape_modes = 0;              // ESCAPED
    bool has_front_pass() const { return kind == JobKind::UTF16 || kind == JobKind::ESCAPED; }
    std::shared_ptr<const RenderSpec> render; // matchy_multi_scanner_set_render, taken by the submit that followed it
    bool is_gz() const { return kind == JobKind::GZ_MEMBERS || kind == JobKind::GZ_FILES || kind == JobKind::GZ_WINDOW || kind == JobKind::GZ_STREAM; }
};
struct MultiDone { int32_t status = MATCHY_SUCCESS; matchy_scan_result_t res{}; const uint8_t* data = nullptr; size_t len = 0; void* tag = nullptr; void* payload = nullptr; size_t worker = 0; };
struct MultiScanner {
    const matchy_t* db = nullptr;
    uint32_t flags = 0;
    std::vector<int> devices;
    std::vector<matchy_scanner_t*> scanners;
    std::vector<std::thread> workers;
    std::mutex mu;
    std::condition_variable cv_work, cv_done, cv_space;
    std::deque<MultiJob> q;
    std::map<size_t, MultiDone> done;
    size_t submitted = 0, taken = 0, max_q = 2;
    // END-TO-END back-pressure (the reference bounds its channels for the same reason, processing/parallel.rs:563-577 "prevent memory
    // explosion"): at most max_inflight batches exist between submit() and next() — queued, being scanned, or finished and not yet
    // taken. Without it a slow consumer of next() (a blocked stdout) lets the reader buffer the whole input and every result.
    size_t max_inflight = 4;
    bool closing = false;
    bool line_ctx = false;   // matchy_multi_scanner_set_line_context: every worker sets its scanner to it before a scan
    bool hit_lines = false;  // matchy_multi_scanner_set_hit_lines: likewise
    bool tally = false, tally_ever = false;   // matchy_multi_scanner_set_tally: likewise
    bool whole_lines = false;   // matchy_multi_scanner_set_whole_lines: likewise
    uint32_t gz_pieces = 0;     // matchy_multi_scanner_set_gz_pieces: likewise, before a gz scan
    std::shared_ptr<const RenderSpec> render_next;   // matchy_multi_scanner_set_render: goes with the next batch submitted
    matchy_multi_batch_fn hook = nullptr;
    void* hook_user = nullptr;
    std::string first_error;   // of a worker (scanner creation, scan): reported through matchy_amd_last_error by next()

    std::vector<int32_t> worker_node, worker_cpus;   // NUMA node of each worker's GPU (-1 unknown), CPUs its thread was bound to (0 = unbound)

    void worker(size_t w) {
        // this thread faults its batches' pages in, pins them and queues their copies: on the NUMA node of its GPU (the binding is
        // taken against the process's affinity at load time, host_topology.cpp: whoever created this thread may have bound itself)
        static const bool no_bind = getenv("MATCHY_AMD_NO_NUMA_BIND") != nullptr;
        {
            const int32_t node = matchy_amd_device_numa_node(devices[w]);
            const int32_t cpus = no_bind ? 0 : matchy_amd_bind_thread_to_device(devices[w]);
            std::lock_guard<std::mutex> lk(mu);
            worker_node[w] = node; worker_cpus[w] = cpus;
        }
        for (;;) {
            MultiJob j{};
            bool want_lines = false, want_hit_lines = false, want_tally = false, touch_tally = false, want_whole_lines = false;
            uint32_t want_gz_pieces = 0;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv_work.wait(lk, [&] { return closing || !q.empty(); });
                if (q.empty()) return;
                // a batch whose bytes live on this worker's node (or anywhere) first — the copy then stays off the socket link; a worker
                // with nothing of its own takes the oldest batch of another node rather than idling
                auto it = q.begin();
                for (auto k = q.begin(); k != q.end(); ++k) if (k->node < 0 || k->node == worker_node[w]) { it = k; break; }
                j = std::move(*it);
                q.erase(it);
                cv_space.notify_one();
                want_lines = line_ctx; want_hit_lines = hit_lines;
                want_tally = tally; touch_tally = tally_ever;
                want_whole_lines = whole_lines;
                want_gz_pieces = gz_pieces;
            }
            MultiDone d;
            d.data = j.data; d.len = j.len; d.tag = j.tag; d.worker = w;
            if (!scanners[w]) scanners[w] = matchy_scanner_create(db, flags, devices[w]);
            std::string err;
            if (scanners[w]) matchy_scanner_set_whole_lines(scanners[w], want_whole_lines);
            if (!scanners[w]) { d.status = MATCHY_ERROR_IO; err = std::string("multi scanner: no scanner on device ") + std::to_string(devices[w]) + ": " + matchy_amd_last_error(); }
            else if (j.len || j.kind != JobKind::PLAIN) {   // an empty batch with a table is scanned too: its result carries the table
                matchy_scanner_t* sc = scanners[w];
                // an armed gz pack without its text: nothing of it can be counted on the host afterwards, so this scan runs with line context
                // (lines with matches per segment) whatever the setting is; an armed UTF-16 or escaped batch without its text likewise
                matchy_scanner_set_line_context(sc, want_lines || ((j.is_gz() || j.has_front_pass()) && j.render && !j.gz_text));
                matchy_scanner_set_hit_lines(sc, want_hit_lines);
                if (touch_tally) matchy_scanner_set_tally(sc, want_tally);
                if (j.is_gz()) (void)matchy_scanner_set_gz_pieces(sc, want_gz_pieces);   // tested by matchy_multi_scanner_set_gz_pieces
                if (j.kind == JobKind::SEGMENTS) d.status = matchy_scanner_set_segments(sc, j.starts.data(), j.starts.size());
                if (j.render) j.render->arm(sc);
                const matchy_gz_window_t window{j.carry.data(), (uint32_t)j.carry.size(), j.carry_cap, j.window_flags};
                const matchy_gz_stream_window_t stream_window{j.stream_state.get(), j.carry.data(), (uint32_t)j.carry.size(), j.carry_cap, j.stream_text_cap, j.window_flags};
                if (d.status == MATCHY_SUCCESS) switch (j.kind) {
                    case JobKind::PLAIN: case JobKind::SEGMENTS: d.status = matchy_scanner_scan(sc, j.data, j.len, &d.res); break;
                    case JobKind::GZ_MEMBERS: d.status = matchy_scanner_scan_gz(sc, j.data, j.len, j.gz.data(), j.gz.size(), MATCHY_SCAN_FETCH_SORTED, j.gz_text, &d.res); break;
                    case JobKind::GZ_FILES: d.status = matchy_scanner_scan_gz_files(sc, j.data, j.len, j.gz_files.data(), j.gz_files.size(), MATCHY_SCAN_FETCH_SORTED, j.gz_text, &d.res); break;
                    case JobKind::GZ_WINDOW: d.status = matchy_scanner_scan_gz_window(sc, j.data, j.len, &window, MATCHY_SCAN_FETCH_SORTED, j.gz_text, &d.res); break;
                    case JobKind::GZ_STREAM: d.status = matchy_scanner_scan_gz_stream(sc, j.data, j.len, &stream_window, MATCHY_SCAN_FETCH_SORTED, j.gz_text, &d.res); break;
                    case JobKind::UTF16: d.status = matchy_scanner_scan_utf16(sc, j.data, j.len, j.byte_order, MATCHY_SCAN_FETCH_SORTED, j.gz_text, &d.res); break;
                    case JobKind::ESCAPED: d.status = matchy_scanner_scan_escaped(sc, j.data, j.len, j.unescape_modes, MATCHY_SCAN_FETCH_SORTED, j.gz_text, &d.res); break;
                }
                if (j.has_front_pass()) {   // the batch's data / len become the text the pass wrote, which the result owns
                    d.data = nullptr; d.len = 0;
                    if (d.status == MATCHY_SUCCESS && j.kind == JobKind::UTF16) (void)matchy_scan_result_utf16(&d.res, &d.data, &d.len, nullptr, nullptr);
                    if (d.status == MATCHY_SUCCESS && j.kind == JobKind::ESCAPED) (void)matchy_scan_result_unescaped(&d.res, &d.data, &d.len, nullptr);
                }
                if (j.is_gz()) {   // the batch's data / len become the inflated text, which the result owns
                    d.data = nullptr; d.len = 0;
                    if (d.status == MATCHY_SUCCESS) (void)matchy_scan_result_gz(&d.res, nullptr, nullptr, &d.data, &d.len);
                }
                if (d.status != MATCHY_SUCCESS) err = matchy_amd_last_error();
            }
            if (d.status == MATCHY_SUCCESS && hook) d.payload = hook(hook_user, w, scanners[w], &d.res, d.data, d.len, j.tag);
            if (j.pinned) matchy_amd_host_unregister(j.pinned);   // behind the hook: the unpin of this batch then runs beside the next worker's copy, not in front of this one's per-hit work
            std::lock_guard<std::mutex> lk(mu);
            if (!err.empty() && first_error.empty()) first_error = err;
            done.emplace(j.seq, d);
            cv_done.notify_all();
        }
    }
};
}  // namespace

extern "C" {

int32_t matchy_amd_device_numa_node(int32_t device) {
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus), device) != hipSuccess) { (void)hipGetLastError(); return -1; }
    return mxy::numa_node_of_pci("/sys", bus);
}
int32_t matchy_amd_bind_thread_to_device(int32_t device) {
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus), device) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return mxy::bind_calling_thread(mxy::cpus_near_pci("/sys", bus));
}
int32_t matchy_amd_unbind_thread(void) { return mxy::unbind_calling_thread(); }
int32_t matchy_amd_numa_cpus(const char* sysfs_root, const char* pci_bus_id, int32_t* out, size_t cap) {
    if (!sysfs_root || !pci_bus_id) return -1;
    const std::vector<int> cpus = mxy::cpus_near_pci(sysfs_root, pci_bus_id);
    if (out) for (size_t i = 0; i < cpus.size() && i < cap; ++i) out[i] = cpus[i];
    return (int32_t)cpus.size();
}

matchy_multi_scanner_t* matchy_multi_scanner_create(const matchy_t* db, uint32_t extract_flags, const int32_t* devices, size_t n_devices) {
    if (!db) return nullptr;
    auto ms = std::make_unique<MultiScanner>();
    ms->db = db; ms->flags = extract_flags;
    if (!devices || !n_devices) ms->devices.push_back(default_device_of(db));
    else for (size_t i = 0; i < n_devices; ++i) { if (devices[i] < 0) { set_error("matchy_multi_scanner_create: negative device"); return nullptr; } ms->devices.push_back(devices[i]); }
    ms->scanners.assign(ms->devices.size(), nullptr);
    ms->worker_node.assign(ms->devices.size(), -1);
    ms->worker_cpus.assign(ms->devices.size(), 0);
    ms->max_q = ms->devices.size() + 1;
    ms->max_inflight = 2 * ms->devices.size() + 2;
    // the first scanner now, so that a database or device that cannot be used fails here; the others are created by their workers
    // when the first batch reaches them (a small input never pays for scanners it does not use)
    ms->scanners[0] = matchy_scanner_create(db, extract_flags, ms->devices[0]);
    if (!ms->scanners[0]) return nullptr;
    MultiScanner* raw = ms.get();
    for (size_t w = 0; w < ms->devices.size(); ++w) ms->workers.emplace_back([raw, w] { raw->worker(w); });
    return reinterpret_cast<matchy_multi_scanner_t*>(ms.release());
}
void matchy_multi_scanner_free(matchy_multi_scanner_t* h) {
    if (!h) return;
    MultiScanner* ms = reinterpret_cast<MultiScanner*>(h);
    { std::lock_guard<std::mutex> lk(ms->mu); ms->closing = true; ms->cv_work.notify_all(); }
    for (auto& t : ms->workers) t.join();
    for (auto& kv : ms->done) matchy_scan_result_free(&kv.second.res);   // results nobody took
    for (auto* sc : ms->scanners) if (sc) matchy_scanner_free(sc);
    delete ms;
}
size_t matchy_multi_scanner_workers(const matchy_multi_scanner_t* h) { return h ? reinterpret_cast<const MultiScanner*>(h)->devices.size() : 0; }
matchy_scanner_t* matchy_multi_scanner_worker_scanner(const matchy_multi_scanner_t* h, size_t worker) {
    const MultiScanner* ms = reinterpret_cast<const MultiScanner*>(h);
    return ms && worker < ms->scanners.size() ? ms->scanners[worker] : nullptr;
}
void matchy_multi_scanner_set_line_context(matchy_multi_scanner_t* h, bool enabled) {
    if (!h) return;
    MultiScanner* ms = reinterpret_cast<MultiScanner*>(h);
    std::lock_guard<std::mutex> lk(ms->mu);
    ms->line_ctx = enabled;
}
void matchy_multi_scanner_set_hit_lines(matchy_multi_scanner_t* h, bool enabled) {
    if (!h) return;
    MultiScanner* ms = reinterpret_cast<MultiScanner*>(h);
    std::lock_guard<std::mutex> lk(ms->mu);
    ms->hit_lines = enabled;
}
int32_t matchy_multi_scanner_set_gz_pieces(matchy_multi_scanner_t* h, uint32_t piece_bytes) {
    if (!h) return MATCHY_ERROR_INVALID_PARAM;
    if (piece_bytes && !gz_piece_bytes_valid(piece_bytes)) { set_error("matchy_multi_scanner_set_gz_pieces: piece_bytes is 0 or a power of two from 512 to 1 MiB"); return MATCHY_ERROR_INVALID_PARAM; }
    MultiScanner* ms = reinterpret_cast<MultiScanner*>(h);
    std::lock_guard<std::mutex> lk(ms->mu);
    ms->gz_pieces = piece_bytes;
    return MATCHY_SUCCESS;
}
// Rendered records: the parameters arm the NEXT batch submitted (whichever submit call that is) and no other; the worker that takes
// the batch arms its scanner with them. The result of the batch owns the block (matchy_scan_result_ndjson).
int32_t matchy_multi_scanner_set_render(matchy_multi_scanner_t* h, const matchy_render_params_t* p) {
    if (!h) return MATCHY_ERROR_INVALID_PARAM;
    MultiScanner* ms = reinterpret_cast<MultiScanner*>(h);
    std::shared_ptr<RenderSpec> spec;
    if (p) {
        if (p->flags & ~(MATCHY_RENDER_LINE_NUMBERS | MATCHY_RENDER_INPUT_LINE)) { set_error("matchy_multi_scanner_set_render: unknown flags"); return MATCHY_ERROR_INVALID_PARAM; }
        if (p->sources && !p->n_sources) { set_error("matchy_multi_scanner_set_render: sources without n_sources"); return MATCHY_ERROR_INVALID_PARAM; }
        spec = std::make_shared<RenderSpec>();
        spec->flags = p->flags;
        if (p->sources) {
            spec->per_segment = true;
            for (size_t k = 0; k < p->n_sources; ++k) { spec->sources.push_back(p->sources[k] ? p->sources[k] : "-"); spec->line_bases.push_back(p->line_bases ? p->line_bases[k] : 0); }
        } else { spec->sources.push_back(p->source ? p->source : "-"); spec->line_bases.push_back(p->line_base); }
    }
    std::lock_guard<std::mutex> lk(ms->mu);
    ms->render_next = std::move(spec);
    return MATCHY_SUCCESS;
}
// Hit tally: the workers switch their scanners' tallies before a scan, like line context; the read-out and the reset touch the scanners
// themselves and therefore need the workers idle (nothing pending).
int32_t matchy_multi_scanner_set_tally(matchy_multi_scanner_t* h, bool enabled) {
    if (!h) return MATCHY_ERROR_INVALID_PARAM;
    MultiScanner* ms = reinterpret_cast<MultiScanner*>(h);
    std::lock_guard<std::mutex> lk(ms->mu);
    ms->tally = enabled;
    if (enabled) ms->tally_ever = true;
    return MATCHY_SUCCESS;
}
// Whole-line queries: the workers switch their scanners before a scan; the batches in flight keep the mode they were submitted
// under only if nothing is pending when it changes, so the call needs the workers idle.
int32_t matchy_multi_scanner_set_whole_lines(matchy_multi_scanner_t* h, bool enabled) {
    if (!h) return MATCHY_ERROR_INVALID_PARAM;
    MultiScanner* ms = reinterpret_cast<MultiScanner*>(h);
    std::lock_guard<std::mutex> lk(ms->mu);
    if (ms->taken != ms->submitted) { set_error("matchy_multi_scanner_set_whole_lines: batches are still pending"); return MATCHY_ERROR_INVALID_PARAM; }
    ms->whole_lines = enabled;
    return MATCHY_SUCCESS;
}
int32_t matchy_multi_scanner_tally_top(matchy_multi_scanner_t* h, size_t limit, matchy_tally_t* out) {
    if (!h || !out) return MATCHY_ERROR_INVALID_PARAM;
    memset(out, 0, sizeof(*out));
    MultiScanner* ms = reinterpret_cast<MultiScanner*>(h);
    {
        std::lock_guard<std::mutex> lk(ms->mu);
        if (ms->taken != ms->submitted) { set_error("matchy_multi_scanner_tally_top: batches are still pending"); return MATCHY_ERROR_INVALID_PARAM; }
        if (!ms->tally_ever) { set_error("matchy_multi_scanner_tally_top: the tally was never enabled on this scanner"); return MATCHY_ERROR_INVALID_PARAM; }
    }
    try {
        // every worker's whole table, merged by (type, text), then ordered and cut
        std::vector<std::vector<TallyEntry>> parts;
        uint64_t matches = 0;
        for (matchy_scanner_t* sc : ms->scanners) {
            if (!sc) continue;
            std::vector<TallyEntry> rows;
            uint64_t d = 0, m = 0;
            if (!scanner_tally_top(sc, 0, rows, d, m)) continue;   // a worker that has not scanned since the tally was enabled
            matches += m;
            parts.push_back(std::move(rows));
        }
        std::vector<TallyEntry> all = tally_merge(parts);
        const uint64_t distinct = all.size();
        tally_order(all, limit);
        fill_tally(std::move(all), distinct, matches, out);
        return MATCHY_SUCCESS;
    } catch (const HipError& e) { set_error(e.what); return MATCHY_ERROR_IO; }
    catch (const std::exception& e) { set_error(e.what()); return MATCHY_ERROR_IO; }
}
void matchy_multi_scanner_reset_tally(matchy_multi_scanner_t* h) {
    if (!h) return;
    MultiScanner* ms = reinterpret_cast<MultiScanner*>(h);
    { std::lock_guard<std::mutex> lk(ms->mu); if (ms->taken != ms->submitted) { set_error("matchy_multi_scanner_reset_tally: batches are still pending"); return; } }
    for (matchy_scanner_t* sc : ms->scanners) if (sc) matchy_scanner_reset_tally(sc);
}
void matchy_multi_scanner_set_batch_hook(matchy_multi_scanner_t* h, matchy_multi_batch_fn fn, void* user) {
    if (!h) return;
    MultiScanner* ms = reinterpret_cast<MultiScanner*>(h);
    std::lock_guard<std::mutex> lk(ms->mu);
    ms->hook = fn; ms->hook_user = user;
}
int32_t matchy_multi_scanner_submit(matchy_multi_scanner_t* h, const uint8_t* data, size_t len, void* tag, const void* pinned_range) {
    return matchy_multi_scanner_submit_near(h, data, len, tag, pinned_range, -1);
}
int32_t matchy_multi_scanner_worker_numa(const matchy_multi_scanner_t* h, size_t worker, int32_t* node, int32_t* cpus_bound) {
    MultiScanner* ms = const_cast<MultiScanner*>(reinterpret_cast<const MultiScanner*>(h));
    if (!ms || worker >= ms->devices.size()) return MATCHY_ERROR_INVALID_PARAM;
    std::lock_guard<std::mutex> lk(ms->mu);
    if (node) *node = ms->worker_node[worker];
    if (cpus_bound) *cpus_bound = ms->worker_cpus[worker];
    return MATCHY_SUCCESS;
}
// The one way into the queue; the job's tables were copied in front of the lock. Blocks while the job queue is full OR max_inflight
// batches are out (someone has to call matchy_multi_scanner_next: a caller that submits and gathers on ONE thread interleaves the two —
// matchy_multi_scanner_pending() tells it when a next() is due).
static int32_t enqueue(MultiScanner* ms, MultiJob&& j) {
    std::unique_lock<std::mutex> lk(ms->mu);
    ms->cv_space.wait(lk, [&] { return ms->q.size() < ms->max_q && ms->submitted - ms->taken < ms->max_inflight; });
    j.seq = ms->submitted++;
    j.render = std::move(ms->render_next);
    ms->q.push_back(std::move(j));
    ms->cv_work.notify_one();
    return MATCHY_SUCCESS;
}
int32_t matchy_multi_scanner_submit_near(matchy_multi_scanner_t* h, const uint8_t* data, size_t len, void* tag, const void* pinned_range, int32_t numa_node) {
    if (!h || (!data && len) || len > 0xFFFFFFFFull) return MATCHY_ERROR_INVALID_PARAM;
    MultiJob j{JobKind::PLAIN, data, len, tag};
    j.pinned = pinned_range; j.node = numa_node;
    return enqueue(reinterpret_cast<MultiScanner*>(h), std::move(j));
}
int32_t matchy_multi_scanner_submit_segments(matchy_multi_scanner_t* h, const uint8_t* data, size_t len, const uint32_t* starts, size_t n, void* tag,
                                             const void* pinned_range) {
    if (!h || (!data && len) || len > 0xFFFFFFFFull || (!starts && n)) return MATCHY_ERROR_INVALID_PARAM;
    MultiJob j{n ? JobKind::SEGMENTS : JobKind::PLAIN, data, len, tag};   // no table: a plain batch
    j.pinned = pinned_range; j.starts.assign(starts, starts + n);
    return enqueue(reinterpret_cast<MultiScanner*>(h), std::move(j));
}
int32_t matchy_multi_scanner_submit_gz(matchy_multi_scanner_t* h, const uint8_t* packed, size_t packed_len, const matchy_gz_member_t* members, size_t n, bool want_text,
                                       void* tag) {
    if (!h || (!packed && packed_len) || !members || n == 0) { set_error("matchy_multi_scanner_submit_gz: no members"); return MATCHY_ERROR_INVALID_PARAM; }
    MultiJob j{JobKind::GZ_MEMBERS, packed, packed_len, tag};
    j.gz_text = want_text; j.gz.assign(members, members + n);
    return enqueue(reinterpret_cast<MultiScanner*>(h), std::move(j));
}
int32_t matchy_multi_scanner_submit_gz_files(matchy_multi_scanner_t* h, const uint8_t* packed, size_t packed_len, const matchy_gz_file_t* files, size_t n_files,
                                             bool want_text, void* tag) {
    if (!h || (!packed && packed_len) || !files || n_files == 0) { set_error("matchy_multi_scanner_submit_gz_files: no files"); return MATCHY_ERROR_INVALID_PARAM; }
    MultiJob j{JobKind::GZ_FILES, packed, packed_len, tag};
    j.gz_text = want_text; j.gz_files.assign(files, files + n_files);
    return enqueue(reinterpret_cast<MultiScanner*>(h), std::move(j));
}
int32_t matchy_multi_scanner_submit_gz_window(matchy_multi_scanner_t* h, const uint8_t* packed, size_t packed_len, const matchy_gz_window_t* window, bool want_text,
                                              void* tag) {
    if (!h) { set_error("matchy_multi_scanner_submit_gz_window: no scanner"); return MATCHY_ERROR_INVALID_PARAM; }
    if (const char* why = gz_window_refusal(packed, packed_len, window)) { set_error(std::string("matchy_multi_scanner_submit_gz_window: ") + why); return MATCHY_ERROR_INVALID_PARAM; }
    MultiJob j{JobKind::GZ_WINDOW, packed, packed_len, tag};
    j.gz_text = want_text; j.carry_cap = window->carry_cap; j.window_flags = window->flags;
    if (window->carry_len) j.carry.assign(window->carry, window->carry + window->carry_len);
    return enqueue(reinterpret_cast<MultiScanner*>(h), std::move(j));
}
int32_t matchy_multi_scanner_submit_gz_stream(matchy_multi_scanner_t* h, const uint8_t* packed, size_t packed_len, const matchy_gz_stream_window_t* window, bool want_text,
                                              void* tag) {
    if (!h) { set_error("matchy_multi_scanner_submit_gz_stream: no scanner"); return MATCHY_ERROR_INVALID_PARAM; }
    if (const char* why = gz_stream_refusal(packed, packed_len, window)) { set_error(std::string("matchy_multi_scanner_submit_gz_stream: ") + why); return MATCHY_ERROR_INVALID_PARAM; }
    MultiJob j{JobKind::GZ_STREAM, packed, packed_len, tag};
    j.gz_text = want_text; j.carry_cap = window->carry_cap; j.window_flags = window->flags; j.stream_text_cap = window->text_cap;
    if (window->carry_len) j.carry.assign(window->carry, window->carry + window->carry_len);
    if (!(window->flags & MATCHY_STREAM_FIRST)) j.stream_state = std::make_unique<matchy_gz_stream_state_t>(*window->state);
    return enqueue(reinterpret_cast<MultiScanner*>(h), std::move(j));
}
int32_t matchy_multi_scanner_submit_utf16(matchy_multi_scanner_t* h, const uint8_t* data, size_t len, uint32_t byte_order, bool want_text, void* tag,
                                          const void* pinned_range) {
    if (!h) { set_error("matchy_multi_scanner_submit_utf16: no scanner"); return MATCHY_ERROR_INVALID_PARAM; }
    if (const char* why = utf16_refusal(data, len, byte_order)) { set_error(std::string("matchy_multi_scanner_submit_utf16: ") + why); return MATCHY_ERROR_INVALID_PARAM; }
    MultiJob j{JobKind::UTF16, data, len, tag};
    j.pinned = pinned_range; j.gz_text = want_text; j.byte_order = byte_order;
    return enqueue(reinterpret_cast<MultiScanner*>(h), std::move(j));
}
int32_t matchy_multi_scanner_submit_escaped(matchy_multi_scanner_t* h, const uint8_t* data, size_t len, uint32_t modes, bool want_text, void* tag,
                                            const void* pinned_range) {
    if (!h) { set_error("matchy_multi_scanner_submit_escaped: no scanner"); return MATCHY_ERROR_INVALID_PARAM; }
    if (const char* why = unescape_refusal(data, len, modes)) { set_error(std::string("matchy_multi_scanner_submit_escaped: ") + why); return MATCHY_ERROR_INVALID_PARAM; }
    MultiJob j{JobKind::ESCAPED, data, len, tag};
    j.pinned = pinned_range; j.gz_text = want_text; j.unescape_modes = modes;
    return enqueue(reinterpret_cast<MultiScanner*>(h), std::move(j));
}
size_t matchy_multi_scanner_pending(const matchy_multi_scanner_t* h) {
    if (!h) return 0;
    MultiScanner* ms = const_cast<MultiScanner*>(reinterpret_cast<const MultiScanner*>(h));
    std::lock_guard<std::mutex> lk(ms->mu);
    return ms->submitted - ms->taken;
}
size_t matchy_multi_scanner_max_pending(const matchy_multi_scanner_t* h) { return h ? reinterpret_cast<const MultiScanner*>(h)->max_inflight : 0; }
int32_t matchy_multi_scanner_next(matchy_multi_scanner_t* h, matchy_multi_batch_t* out) {
    if (!h || !out) return MATCHY_ERROR_INVALID_PARAM;
    MultiScanner* ms = reinterpret_cast<MultiScanner*>(h);
    std::unique_lock<std::mutex> lk(ms->mu);
    if (ms->taken == ms->submitted) return 0;   // nothing pending
    ms->cv_done.wait(lk, [&] { return ms->done.count(ms->taken) != 0; });
    const MultiDone d = ms->done[ms->taken];
    ms->done.erase(ms->taken);
    out->seq = ms->taken++;
    ms->cv_space.notify_all();
    out->status = d.status; out->result = d.res; out->data = d.data; out->len = d.len; out->tag = d.tag; out->payload = d.payload; out->worker = d.worker;
    if (d.status != MATCHY_SUCCESS) set_error(ms->first_error.empty() ? "multi scanner: a batch failed" : ms->first_error);
    return 1;
}

// One buffer through all workers: cut at newlines into pieces (batch_bytes each; 0 = the buffer spread twice over the workers, at
// least 4 MiB and at most 256 MiB a piece), results merged into ONE result with offsets into `data` — what matchy_scanner_scan
// returns for the same bytes, whatever the device list.
int32_t matchy_multi_scanner_scan(matchy_multi_scanner_t* h, const uint8_t* data, size_t len, size_t batch_bytes, matchy_scan_result_t* out) {
    if (!h || !out || (!data && len) || len > 0xFFFFFFFFull) return MATCHY_ERROR_INVALID_PARAM;
    MultiScanner* ms = reinterpret_cast<MultiScanner*>(h);
    { std::lock_guard<std::mutex> lk(ms->mu); if (ms->taken != ms->submitted) { set_error("matchy_multi_scanner_scan: batches of an earlier submit are still pending"); return MATCHY_ERROR_INVALID_PARAM; } }
    if (!batch_bytes) {
        batch_bytes = (len + 2 * ms->devices.size() - 1) / (2 * ms->devices.size());
        batch_bytes = std::min<size_t>(std::max<size_t>(batch_bytes, (size_t)4 << 20), (size_t)256 << 20);
    }
    auto in = std::make_unique<ScanResultInternal>();
    uint64_t lines = 0, cands = 0;
    int32_t status = MATCHY_SUCCESS;
    std::string err;
    // takes what has finished; the first `must` batches are waited for
    auto take = [&](size_t must) {
        for (;; must -= must ? 1 : 0) {
            { std::lock_guard<std::mutex> lk(ms->mu); if (ms->taken == ms->submitted || (!must && !ms->done.count(ms->taken))) return; }
            matchy_multi_batch_t b;
            if (matchy_multi_scanner_next(h, &b) != 1) return;
            if (b.status != MATCHY_SUCCESS) { if (status == MATCHY_SUCCESS) { status = b.status; err = matchy_amd_last_error(); } }
            else {
                append_shifted(b.result.hits, b.result.n_hits, b.result.pattern_ids, b.result.data_offsets, b.result.n_ids, (uint32_t)(b.data - data),
                               in->hits, in->ids, in->offs);
                // batches come back in submission order and end at line ends: a batch's lines continue the count of the earlier ones
                const ScanResultInternal* bi = reinterpret_cast<const ScanResultInternal*>(b.result._internal);
                if (bi && bi->has_lines) {
                    in->has_lines = true; in->lines_with_matches += bi->lines_with_matches;
                    if (bi->lines) append_shifted_lines(bi->lines, b.result.n_hits, (uint32_t)(b.data - data), (uint32_t)lines, in->lines_own);
                }
                lines += b.result.lines; cands += b.result.candidates;
            }
            matchy_scan_result_free(&b.result);
        }
    };
    for (size_t pos = 0; pos < len;) {
        const size_t end = newline_cut(data, pos, len, batch_bytes);
        // this thread submits AND gathers: make room before a submit that would block on the in-flight bound
        if (matchy_multi_scanner_pending(h) >= ms->max_inflight) take(1);
        const int32_t src = matchy_multi_scanner_submit(h, data + pos, end - pos, nullptr, nullptr);
        if (src != MATCHY_SUCCESS) { if (status == MATCHY_SUCCESS) { status = src; err = "matchy_multi_scanner_scan: a line of 4 GiB or more cannot be submitted"; } break; }
        pos = end;
        take(0);
    }
    take((size_t)-1);
    if (status != MATCHY_SUCCESS) { set_error(err); return status; }
    memset(out, 0, sizeof(*out));
    out->lines = lines; out->candidates = cands; out->bytes = len;
    out->n_hits = in->hits.size(); out->n_ids = in->ids.size();
    out->hits = in->hits.data(); out->pattern_ids = in->ids.data(); out->data_offsets = in->offs.data();
    if (in->has_lines) in->lines = in->lines_own.empty() ? nullptr : in->lines_own.data();
    else if (len == 0) { std::lock_guard<std::mutex> lk(ms->mu); in->has_lines = ms->line_ctx; }   // no batch: the answer is still "0 lines"
    out->_internal = in.release();
    return MATCHY_SUCCESS;
}

// A regular file (mapped; a reader thread cuts it into newline-aligned batches, faults their pages in, pins them and submits them) or a
// stream ("-" = stdin, a pipe: read into buffers of batch_bytes). `fn` is called on the calling thread for every batch IN FILE ORDER
// with the batch's result and its offset in the file (batch->tag); the result is released when fn returns. Compressed inputs are the
// caller's business (decompress and matchy_multi_scanner_submit: `matchy match` does that for .gz). Returns 0, or the first error.
int32_t matchy_multi_scanner_scan_file(matchy_multi_scanner_t* h, const char* path, size_t batch_bytes, matchy_multi_ordered_fn fn, void* user, matchy_multi_totals_t* totals) {
    if (!h || !path) return MATCHY_ERROR_INVALID_PARAM;
    MultiScanner* ms = reinterpret_cast<MultiScanner*>(h);
    { std::lock_guard<std::mutex> lk(ms->mu); if (ms->taken != ms->submitted) { set_error("matchy_multi_scanner_scan_file: batches of an earlier submit are still pending"); return MATCHY_ERROR_INVALID_PARAM; } }
    if (!batch_bytes) batch_bytes = (size_t)256 << 20;
    if (batch_bytes > 0xF0000000ull) batch_bytes = 0xF0000000ull;
    const bool is_stdin = strcmp(path, "-") == 0;
    const int fd = is_stdin ? 0 : open(path, O_RDONLY);
    if (fd < 0) { set_error(std::string("matchy_multi_scanner_scan_file: cannot open ") + path + ": " + strerror(errno)); return MATCHY_ERROR_FILE_NOT_FOUND; }
    struct stat sb;
    const bool regular = !is_stdin && fstat(fd, &sb) == 0 && S_ISREG(sb.st_mode) && sb.st_size > 0;
    void* map = MAP_FAILED;
    size_t map_len = 0;
    if (regular) { map_len = (size_t)sb.st_size; map = mmap(nullptr, map_len, PROT_READ, MAP_PRIVATE, fd, 0); }
    std::atomic<bool> reader_ok{true}, stop{false}, reader_finished{false};
    const bool mapped = map != MAP_FAILED;
    std::thread reader([&] {
        struct Finished { std::atomic<bool>& f; ~Finished() { f = true; } } fin{reader_finished};
        // false ends the reader: the gathering side has an error, or the library did not take the batch (a line of 4 GiB or more)
        auto submit = [&](const uint8_t* p, size_t n, uint64_t off, const void* pinned) {
            const bool stopped = stop;
            if (!stopped && matchy_multi_scanner_submit(h, p, n, (void*)(uintptr_t)off, pinned) == MATCHY_SUCCESS) return true;
            if (pinned) matchy_amd_host_unregister(pinned);
            if (!stopped) reader_ok = false;
            return false;
        };
        if (mapped) {
            (void)madvise(map, map_len, MADV_SEQUENTIAL);
            const uint8_t* base = (const uint8_t*)map;
            for (size_t pos = 0; pos < map_len;) {
                const size_t end = newline_cut(base, pos, map_len, batch_bytes);
                if (!submit(base + pos, end - pos, pos, prefault_and_pin(base + pos, end - pos))) return;
                pos = end;
            }
            return;
        }
        // stream: a submitted buffer belongs to the gathering thread, which frees it when its batch has been handed to the callback
        const StreamEnd e = read_batches([&](void* p, size_t n) { return read(fd, p, n); }, batch_bytes, [&](Bytes&& data, size_t n, uint64_t off) {
            if (!submit(data.get(), n, off, nullptr)) return false;
            data.release();
            return true;
        });
        if (e == StreamEnd::FAILED) reader_ok = false;
    });
    // The calling thread gathers in order while the reader is still submitting. EVERY error ends the same way: `stop` makes the reader
    // end at its next batch, and the loop goes on taking results until the reader has finished and nothing is pending — a reader
    // blocked in submit on the in-flight bound is released by the next take, so the join below cannot wait on it.
    int32_t status = MATCHY_SUCCESS;
    std::string err;
    auto fail = [&](int32_t code, const std::string& what) { if (status == MATCHY_SUCCESS) { status = code; err = what; } stop = true; };
    matchy_multi_totals_t t{};
    for (;;) {
        const bool last = reader_finished;   // read BEFORE the take: nothing is submitted behind it, so an empty take is the end
        matchy_multi_batch_t b;
        const int32_t r = matchy_multi_scanner_next(h, &b);
        if (r != 1) {
            if (r != 0) fail(r, "matchy_multi_scanner_scan_file: gather failed");
            if (last) break;
            std::this_thread::sleep_for(std::chrono::microseconds(200));   // between two submits
            continue;
        }
        if (b.status != MATCHY_SUCCESS) fail(b.status, matchy_amd_last_error());
        else {
            t.batches += 1; t.bytes += b.len; t.lines += b.result.lines; t.candidates += b.result.candidates; t.matches += b.result.n_hits + b.result.n_ip4_hits;
            if (fn && status == MATCHY_SUCCESS) { const int32_t fr = fn(user, &b); if (fr != 0) fail(fr, "matchy_multi_scanner_scan_file: the batch callback asked to stop"); }
        }
        matchy_scan_result_free(&b.result);
        if (!mapped) free(const_cast<uint8_t*>(b.data));
    }
    reader.join();
    if (map != MAP_FAILED) munmap(map, map_len);
    if (!is_stdin) close(fd);
    if (totals) *totals = t;
    if (!reader_ok && status == MATCHY_SUCCESS) { status = MATCHY_ERROR_IO; err = std::string("matchy_multi_scanner_scan_file: reading ") + path + " failed"; }
    if (status != MATCHY_SUCCESS) set_error(err);
    return status;
}

}  // extern "C"
