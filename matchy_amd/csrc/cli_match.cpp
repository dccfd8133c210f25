// `match` prints one JSON object per match on stdout (same records as the reference's parallel path,
// match_processor/parallel.rs:297-369: sorted keys, timestamp "0.000") and, with -s, the [INFO] statistics block on
// stderr (commands/match_cmd.rs:514-581). Every batch is scanned on the GPU through the C ABI (matchy_scanner_scan);
// there is no CPU scan path. Flags that only tune the reference's CPU thread pool (-j, --readers, --cache-size, -p,
// --debug-routing) are accepted and ignored; .gz inputs are decompressed on the host (zlib); -f/--follow polls the files.
// --tally[=N] adds, behind the match records, {"count","item_type","matched_text","result"} per distinct matched value (tally.hip).
// --pack-inputs reads consecutive small input files into shared batches (input_packer.h) and scans each as one batch of segments
// (segments.hip): the output is byte for byte what it is without the flag.
// --gz-on-gpu sends runs of consecutive small .gz inputs to the GPU compressed (matchy_multi_scanner_submit_gz, inflate.hip): one wave
// per file inflates them into the segments of one batch. A file the GPU does not accept (a second member, a damaged stream) is read the
// old way right behind its pack, so it is scanned or reported exactly as without the flag; only its place in the output moves.
// --gz-members (with --gz-on-gpu) extends the packs to .gz files of many small members that fit one batch
// (matchy_multi_scanner_submit_gz_files): one wave per member, the file is one segment, the verdict is per file.
// --gz-windows (with both) extends that to multi-member .gz files LARGER than a batch: the mapped file goes out as a chain of windows of
// whole members (matchy_multi_scanner_submit_gz_window), one at a time; every window hands the partial line behind its last '\n' to the next.
// --gz-stream-windows (with --gz-on-gpu --gz-pieces) does the same for a .gz file of ONE member that does not fit a batch: a chain of
// windows of its DEFLATE stream (matchy_multi_scanner_submit_gz_stream; gz_stream.h walks it), each handing the bit it stopped at, the
// CRC and length so far and the last 32 KiB of text to the next, with the partial line.
// --encoding=utf-16le|utf-16be|auto sends the batches of UTF-16 inputs to the GPU as they are (matchy_multi_scanner_submit_utf16, utf16.hip):
// cut behind 000A units (newline_cut16), transcoded to UTF-8 there and scanned; records, offsets and lines are those of the UTF-8 text.
// --unescape=percent|json|json+percent sends the batches of every input — read as bytes and cut behind LF as ever — to the GPU to be decoded
// in front of the scan (matchy_multi_scanner_submit_escaped, unescape.hip): records and offsets are those of the decoded text, and since an
// escape for LF becomes a space, line numbers are those of the input.
#include <fcntl.h>
#include <signal.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>
#include <ctime>

#include "cli_common.h"
#include "batch_reader.h"
#include "gz_packer.h"
#include "gz_stream.h"

using namespace mxy;

namespace {

struct Totals {
    unsigned long long lines = 0, lines_with_matches = 0, matches = 0, candidates = 0, bytes = 0;
    Totals& operator+=(const Totals& o) { lines += o.lines; lines_with_matches += o.lines_with_matches; matches += o.matches; candidates += o.candidates; bytes += o.bytes; return *this; }
};

// --gz-on-gpu: the statuses of a pack's files (MATCHY_GZ_*) on their way from the worker that scanned the pack to the reader, which
// reads the files that failed the old way before it submits anything else
struct GzVerdict {
    std::mutex mu;
    std::condition_variable cv;
    bool done = false;
    std::vector<int32_t> status;   // empty with done set: the pack was not scanned at all, every member is read the old way
    // --gz-windows: MATCHY_WINDOW_*, the carry for the next window and the bytes of the file this window consumed; written before set()
    int32_t window_status = MATCHY_WINDOW_OK;
    std::vector<uint8_t> carry;
    uint64_t bytes = 0;
    // --gz-stream-windows: MATCHY_STREAM_*, where the window stopped, and the state for the next window; written before set()
    int32_t stream_status = MATCHY_STREAM_OK;
    uint64_t consumed_bits = 0;
    uint32_t text_len = 0;
    bool ended = false;
    std::shared_ptr<matchy_gz_stream_state_t> state;
    void set(const int32_t* st, size_t n) {
        { std::lock_guard<std::mutex> lk(mu); if (done) return; status.assign(st, st + n); done = true; }
        cv.notify_all();
    }
    void wait() { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return done; }); }
};

// ---- `matchy match`: reader -> batches -> one worker per device entry -> ordered printer
// The pipeline itself is the library's (matchy_multi_scanner_*: one worker thread and scanner per device entry, batches handed out in
// sequence, results taken back in sequence — processing/parallel.rs:494-505 behind the C ABI). What stays here is what belongs to
// the command line: the reader cuts every input into newline-aligned batches (FileReader::next_batch, processing/mod.rs:206-251;
// regular files are mapped, .gz / stdin are read), the batch hook renders a batch's matches on the worker that scanned it, and the
// printer emits the rendered batches in sequence order, so the output is the same for every device list (line blocks
// are independent, the database is replicated, the host gathers the hit records and sums the counters; no collective).
// STREAM: a newline-aligned piece of one input. PACK (--pack-inputs): several files, one segment each. GZ_PACK (--gz-on-gpu): gzip files,
// compressed, one segment each. GZ_WINDOW (--gz-windows): one window of whole members of one gzip file: ONE segment like a pack of one
// file, but its lines count on from those of the windows in front. GZ_STREAM (--gz-stream-windows): one window of ONE DEFLATE stream, a
// segment whose lines count on in the same way.
// UTF16 (--encoding): a piece of one UTF-16 input that ends behind a 000A unit; what comes back is its UTF-8 text.
// ESCAPED (--unescape): a newline-aligned piece of one input, like STREAM; what comes back is its decoded text.
enum class BatchKind { STREAM, PACK, GZ_PACK, GZ_WINDOW, GZ_STREAM, UTF16, ESCAPED };
// --encoding: how the bytes of an input are read. AUTO decides per input by its first two bytes (FF FE / FE FF, else BYTES).
enum class Encoding { BYTES, UTF16LE, UTF16BE, AUTO };
struct Batch {
    BatchKind kind = BatchKind::STREAM;
    size_t input = 0;                   // the input of a stream batch or a window; the first of a pack
    Bytes own;
    const uint8_t* ptr = nullptr;       // into `own` (inputs that are read: stdin, .gz, packs) or into a file mapping that outlives the batch
    size_t len = 0;
    const void* reg = nullptr;          // page range of a batch the reader pinned ahead of the scan (unpinned by the worker)
    std::vector<PackedInput> pack;      // PACK: its files
    size_t appended = 0;                // PACK: the newlines the packer added
    std::vector<GzFile> gz;             // GZ_PACK: its files, end to end in `ptr`; GZ_WINDOW: gz[0] is the window
    std::shared_ptr<GzVerdict> verdict; // GZ_PACK, GZ_WINDOW: where the reader waits for the verdict on them
    std::vector<uint8_t> carry;         // GZ_WINDOW, GZ_STREAM: the partial line the window in front left behind
    uint32_t carry_cap = 0;             // GZ_WINDOW, GZ_STREAM
    std::shared_ptr<matchy_gz_stream_state_t> stream_state;   // GZ_STREAM: the state the window in front handed out (none for the first)
    uint32_t stream_text_cap = 0, stream_flags = 0;           // GZ_STREAM: MATCHY_STREAM_*
    bool window_last = false;           // GZ_WINDOW: the file ends with this window
    uint32_t byte_order = 0;            // UTF16: MATCHY_UTF16_*
    uint32_t unescape_modes = 0;        // ESCAPED: MATCHY_UNESCAPE_*
    bool armed = false;                 // --render-on-gpu: the batch was submitted with matchy_multi_scanner_set_render

    bool is_gz() const { return kind == BatchKind::GZ_PACK || kind == BatchKind::GZ_WINDOW || kind == BatchKind::GZ_STREAM; }
    bool front_pass() const { return kind == BatchKind::UTF16 || kind == BatchKind::ESCAPED; }   // the scan runs over a text made from the batch on the device
    bool segmented() const { return kind != BatchKind::STREAM && !front_pass(); }   // the scan result carries a segment table
    // the batch's text is made on the device: it comes back only where wants_text says so
    bool text_on_device() const { return is_gz() || front_pass(); }
    // the batch goes on where its input's earlier batches ended: only the first has line base 0 (every segment of a pack is a whole file)
    bool continues_lines() const { return kind == BatchKind::STREAM || front_pass() || kind == BatchKind::GZ_WINDOW || kind == BatchKind::GZ_STREAM; }
    // a gz, UTF-16 or escaped batch: its text comes back only where something is rendered from it on the host
    bool wants_text(bool json, bool gather) const { return json && !gather && !armed; }
    // every input the batch carries, in segment order
    template <class F> void each_input(F&& f) const {
        switch (kind) {
            case BatchKind::STREAM: case BatchKind::UTF16: case BatchKind::ESCAPED: f(input); break;
            case BatchKind::PACK: for (const PackedInput& pi : pack) f(pi.input); break;
            case BatchKind::GZ_PACK: case BatchKind::GZ_WINDOW: case BatchKind::GZ_STREAM: for (const GzFile& g : gz) f(g.input); break;
        }
    }
};
// what a batch contributes to the output: `text` / `text_len` is the buffer matchy_scan_result_to_ndjson returned (written to stdout as
// it is and released by the printer: 200 bytes per match are not copied again on the way), `out` what --follow builds from it
struct Done {
    std::string out; char* text = nullptr; size_t text_len = 0; Totals t; bool ok = true;
    bool skip = false;   // nothing of the batch is printed from its result: its inputs are read again the old way
    Done() = default;
    Done(const Done&) = delete;
    Done& operator=(const Done&) = delete;
    ~Done() { if (text) matchy_free_string(text); }
};
// all of a buffer to stdout, past stdio (a gigabyte of NDJSON per ten gigabytes of log need not pass through its buffer)
static void write_all_stdout(const char* p, size_t n) {
    fflush(stdout);
    while (n) {
        const ssize_t w = write(1, p, n);
        if (w < 0) { if (errno == EINTR) continue; return; }
        p += w; n -= (size_t)w;
    }
}

struct MatchPipeline {
    matchy_multi_scanner_t* ms = nullptr;
    std::mutex mu;
    size_t submitted = 0;
    std::atomic<bool> reader_done{false};
    bool json = true;
    std::vector<std::string> sources;
    // --line-numbers / --input-line: the scanners run with line context. "Lines with matches" is the device's count, and the records
    // carry "line_number" (1-based per input) — which needs the number of lines in front of the batch, known only in sequence order:
    // such batches are rendered by the ordered printer (line_base: '\n' bytes of the input's earlier batches; batches end at newlines),
    // not by the batch hook.
    bool line_ctx = false, input_line = false;
    // --gather-lines: the scanners run with hit lines. Every result carries the lines of its matches, the renderers read those (the
    // text of a gz pack stays on the device), and "Lines with matches" is the device's count as with line context.
    bool gather = false;
    // --gz-members: gz packs hold files of one member or many (matchy_multi_scanner_submit_gz_files); the verdicts are per file
    bool gz_members = false;
    // --render-on-gpu: a batch whose line bases are known when it is submitted leaves the device as finished NDJSON
    // (matchy_multi_scanner_set_render): every batch without line numbers; with them the packs (every segment is a whole file: base 0)
    // and an input's first batch. Any other batch, and a batch whose render status is not OK, goes through the host renderer as before.
    bool render_gpu = false;
    std::vector<char> input_started;   // the reader's: the input has had a batch submitted
    std::atomic<size_t> gpu_batches{0}, gpu_fallback{0};
    std::atomic<unsigned long long> gpu_bytes{0};
    // --whole-lines: the scanners' counters of every batch (queries, address, string, invalid UTF-8), summed for -s
    bool whole_lines = false;
    std::atomic<unsigned long long> wl_counters[4] = {{0}, {0}, {0}, {0}};
    void add_whole_lines(const matchy_scanner_t* sc) {
        uint64_t c[4] = {0, 0, 0, 0};
        matchy_scanner_get_whole_lines_counters(sc, c);
        for (int k = 0; k < 4; ++k) wl_counters[k] += c[k];
    }
    // --encoding: what the UTF-16 batches say about themselves, summed for -s (the times: count, prefix, write)
    std::atomic<size_t> u16_inputs{0}, u16_batches{0};
    std::atomic<unsigned long long> u16_units{0}, u16_replaced{0};
    double u16_ms[3] = {0, 0, 0};   // guarded by mu
    void add_utf16(const matchy_scanner_t* sc, const matchy_scan_result_t& r) {
        uint64_t units = 0, replaced = 0;
        float ms[3] = {0, 0, 0};
        if (matchy_scan_result_utf16(&r, nullptr, nullptr, &units, &replaced) != MATCHY_SUCCESS) return;
        matchy_scanner_get_utf16_timing(sc, ms);
        ++u16_batches; u16_units += units; u16_replaced += replaced;
        std::lock_guard<std::mutex> lk(mu);
        for (int k = 0; k < 3; ++k) u16_ms[k] += ms[k];
    }
    // --unescape: the modes of every batch that is read as bytes (0: off), and what the decoded batches say about themselves, summed for -s
    uint32_t unescape_modes = 0;
    std::atomic<size_t> ue_batches{0};
    std::atomic<unsigned long long> ue_in_bytes{0}, ue_text_bytes{0}, ue_counters[3] = {{0}, {0}, {0}};
    double ue_ms[3] = {0, 0, 0};   // guarded by mu
    void add_unescaped(const matchy_scanner_t* sc, const matchy_scan_result_t& r, size_t in_len) {
        uint64_t c[3] = {0, 0, 0};
        size_t text_len = 0;
        float ms[3] = {0, 0, 0};
        if (matchy_scan_result_unescaped(&r, nullptr, &text_len, c) != MATCHY_SUCCESS) return;
        matchy_scanner_get_unescape_timing(sc, ms);
        ++ue_batches; ue_in_bytes += in_len; ue_text_bytes += text_len;
        for (int k = 0; k < 3; ++k) ue_counters[k] += c[k];
        std::lock_guard<std::mutex> lk(mu);
        for (int k = 0; k < 3; ++k) ue_ms[k] += ms[k];
    }
    std::vector<unsigned long long> line_base;   // per input; the printer's (then --follow's)
    // arms the library for the batch about to be submitted, where its line bases are known
    void arm(Batch& b) {
        if (!render_gpu || !json) return;
        bool first = true;
        if (b.continues_lines()) {
            if (input_started.size() <= b.input) input_started.resize(b.input + 1, 0);
            first = !input_started[b.input];
            input_started[b.input] = 1;
        }
        if (line_ctx && !first) return;
        matchy_render_params_t p;
        memset(&p, 0, sizeof(p));
        p.flags = line_ctx ? (MATCHY_RENDER_LINE_NUMBERS | (input_line ? MATCHY_RENDER_INPUT_LINE : 0u)) : 0u;
        std::vector<const char*> src;
        if (b.segmented()) { src = pack_sources(b); p.sources = src.data(); p.n_sources = src.size(); }
        else p.source = sources[b.input].c_str();
        b.armed = matchy_multi_scanner_set_render(ms, &p) == MATCHY_SUCCESS;   // copied at the call
    }
    // the block of an armed batch as the text of its Done; false: not rendered there (the host renderer takes over)
    bool take_gpu_text(const matchy_scan_result_t& r, Done& d) {
        const char* text = nullptr;
        uint64_t n = 0;
        int32_t status = MATCHY_RENDER_OK;
        if (matchy_scan_result_ndjson(&r, &text, &n, &status) != MATCHY_SUCCESS || status != MATCHY_RENDER_OK) { ++gpu_fallback; return false; }
        if (n) {
            char* copy = (char*)malloc(n);   // the result goes when the hook returns; the printer frees this like the host renderer's buffer
            if (!copy) { ++gpu_fallback; return false; }
            memcpy(copy, text, n);
            d.text = copy; d.text_len = n;
        }
        ++gpu_batches; gpu_bytes += n;
        return true;
    }

    // the batch goes to the library's queue; its Batch object travels as the tag and comes back with the result
    size_t submit(Batch&& b) {
        Batch* hb = new Batch(std::move(b));
        size_t seq;
        { std::lock_guard<std::mutex> lk(mu); seq = submitted++; }
        int32_t rc = MATCHY_ERROR_INVALID_PARAM;
        arm(*hb);
        const bool text = hb->wants_text(json, gather);
        switch (hb->kind) {
            case BatchKind::STREAM: rc = matchy_multi_scanner_submit(ms, hb->ptr, hb->len, hb, hb->reg); break;
            case BatchKind::UTF16: rc = matchy_multi_scanner_submit_utf16(ms, hb->ptr, hb->len, hb->byte_order, text, hb, hb->reg); break;
            case BatchKind::ESCAPED: rc = matchy_multi_scanner_submit_escaped(ms, hb->ptr, hb->len, hb->unescape_modes, text, hb, hb->reg); break;
            case BatchKind::PACK: {
                std::vector<uint32_t> starts;
                for (const PackedInput& pi : hb->pack) starts.push_back(pi.start);
                rc = matchy_multi_scanner_submit_segments(ms, hb->ptr, hb->len, starts.data(), starts.size(), hb, hb->reg);
                break;
            }
            case BatchKind::GZ_PACK:
                if (gz_members) {
                    std::vector<matchy_gz_file_t> table;
                    for (const GzFile& g : hb->gz) table.push_back(matchy_gz_file_t{g.offset, g.len});
                    rc = matchy_multi_scanner_submit_gz_files(ms, hb->ptr, hb->len, table.data(), table.size(), text, hb);
                } else {
                    std::vector<matchy_gz_member_t> table;
                    for (const GzFile& g : hb->gz) table.push_back(matchy_gz_member_t{g.offset, g.len, 0});
                    rc = matchy_multi_scanner_submit_gz(ms, hb->ptr, hb->len, table.data(), table.size(), text, hb);
                }
                break;
            case BatchKind::GZ_WINDOW: {
                const matchy_gz_window_t w{hb->carry.data(), (uint32_t)hb->carry.size(), hb->carry_cap, hb->window_last ? MATCHY_WINDOW_LAST : 0u};
                rc = matchy_multi_scanner_submit_gz_window(ms, hb->ptr, hb->len, &w, text, hb);
                break;
            }
            case BatchKind::GZ_STREAM: {
                const matchy_gz_stream_window_t w{hb->stream_state.get(), hb->carry.data(), (uint32_t)hb->carry.size(), hb->carry_cap, hb->stream_text_cap, hb->stream_flags};
                rc = matchy_multi_scanner_submit_gz_stream(ms, hb->ptr, hb->len, &w, text, hb);
                break;
            }
        }
        if (rc == MATCHY_SUCCESS) return seq;
        // not queued (cannot happen for batches below 4 GiB): the printer never sees it
        matchy_multi_scanner_set_render(ms, nullptr);   // the parameters go with a batch that was queued, never with the next one
        if (hb->is_gz()) hb->verdict->set(nullptr, 0);   // every file goes the old way
        else {
            fprintf(stderr, "[ERROR] batch of %zu bytes rejected: %s\n", hb->len, matchy_amd_last_error());
            { std::lock_guard<std::mutex> lk(mu); hb->each_input([&](size_t i) { rejected_inputs.push_back(i); }); }   // its matches are missing: the inputs count as failed
            if (hb->reg) matchy_amd_host_unregister(hb->reg);
        }
        delete hb;
        return seq;
    }
    // Mapped inputs: the mapping of a file is released by the printer as soon as the file's last batch has been printed — the
    // page tables of a file of gigabytes take tens of milliseconds to tear down, and that runs beside the scans of the next
    // files instead of behind the last one.
    // bytes of each input the first pass has read: where --follow starts watching (a size taken AFTER that pass would skip what was appended in between)
    std::vector<long long> consumed;
    std::vector<size_t> rejected_inputs;   // guarded by mu: inputs with a batch the library did not take
    struct Mapping { void* p; size_t len; size_t last_seq; bool released; };
    std::vector<Mapping> mappings;   // guarded by mu
    void add_mapping(void* p, size_t len, size_t last_seq) { std::lock_guard<std::mutex> lk(mu); mappings.push_back({p, len, last_seq, false}); }
    void release_mappings(size_t printed_below) {   // every batch with seq < printed_below is done
        std::vector<Mapping> go;
        {
            std::lock_guard<std::mutex> lk(mu);
            for (Mapping& m : mappings) if (!m.released && m.last_seq < printed_below) { m.released = true; go.push_back(m); }
        }
        for (const Mapping& m : go) munmap(m.p, m.len);
    }
    // what one batch contributes to the output: counters, and (json) its matches rendered — on the worker thread that scanned it
    void render(matchy_scanner_t* sc, const matchy_scan_result_t& r, const uint8_t* data, size_t len, const Batch& b, Done& d) {
        Totals& t = d.t;
        if (b.is_gz() && b.armed && data == nullptr) {
            // an armed gz pack came without its text: where its block is not to be had nothing can be rendered from it, and every
            // member is read the old way, as if the GPU had accepted none
            int32_t status = MATCHY_RENDER_OK;
            if (matchy_scan_result_ndjson(&r, nullptr, nullptr, &status) != MATCHY_SUCCESS || status != MATCHY_RENDER_OK) { ++gpu_fallback; d.skip = true; b.verdict->set(nullptr, 0); return; }
        }
        if (b.is_gz()) {
            // a gz pack: lines and bytes are those of the members the GPU accepted (separators and the regions of the others are not
            // counted); the others are read the old way by the reader, which waits for this verdict
            t.lines += r.lines; t.candidates += r.candidates; t.bytes += r.bytes; t.matches += r.n_hits;
            const int32_t* st = nullptr;
            size_t n_st = 0;
            const int32_t got = gz_members && b.kind != BatchKind::GZ_STREAM ? matchy_scan_result_gz_files(&r, &st, &n_st, nullptr) : matchy_scan_result_gz(&r, &st, &n_st, nullptr, nullptr);   // per file either way
            if (got != MATCHY_SUCCESS) { st = nullptr; n_st = 0; d.ok = false; }
            if (b.kind == BatchKind::GZ_WINDOW && got == MATCHY_SUCCESS) {
                const uint8_t* carry = nullptr;
                size_t n_carry = 0;
                if (matchy_scan_result_gz_window(&r, &b.verdict->window_status, &carry, &n_carry) == MATCHY_SUCCESS) { b.verdict->carry.assign(carry, carry + n_carry); b.verdict->bytes = r.bytes; }
                else { st = nullptr; n_st = 0; d.ok = false; }
            }
            if (b.kind == BatchKind::GZ_STREAM && got == MATCHY_SUCCESS) {
                GzVerdict& v = *b.verdict;
                const matchy_gz_stream_state_t* state = nullptr;
                const uint8_t* carry = nullptr;
                size_t n_carry = 0;
                if (matchy_scan_result_gz_stream(&r, &v.stream_status, nullptr, &v.consumed_bits, &v.text_len, &v.ended, &state, &carry, &n_carry) == MATCHY_SUCCESS) {
                    v.carry.assign(carry, carry + n_carry); v.bytes = r.bytes;
                    if (state) v.state = std::make_shared<matchy_gz_stream_state_t>(*state);
                } else { st = nullptr; n_st = 0; d.ok = false; }
            }
            b.verdict->set(st, n_st);
            if (!d.ok) { fprintf(stderr, "[ERROR] no gz statuses in the scan result of a gz pack: %s\n", matchy_amd_last_error()); return; }
        } else {
            // a pack: the newlines the packer appended are not the inputs'
            t.lines += r.lines - b.appended; t.candidates += r.candidates; t.bytes += len - b.appended; t.matches += r.n_hits;
        }
        // an armed gz pack comes back without its text: the library scans it with line context, and its "Lines with matches" are the
        // table's like those of any pack scanned with line context (plain batches of the same run are counted from their text as before)
        // (an armed UTF-16 or escaped batch likewise: its count is the scan's own)
        const bool table_counts = line_ctx || gather || (b.armed && b.text_on_device());
        if (table_counts && b.segmented()) {   // per segment, from the table the GPU filled
            const matchy_scan_segment_t* segs = nullptr;
            size_t n_segs = 0;
            if (matchy_scan_result_segments(&r, nullptr, nullptr, &segs, &n_segs) == MATCHY_SUCCESS) for (size_t k = 0; k < n_segs; ++k) t.lines_with_matches += segs[k].lines_with_matches;
            else { fprintf(stderr, "[ERROR] no segments in the scan result of a pack: %s\n", matchy_amd_last_error()); d.ok = false; }
            if (line_ctx || !d.ok) return;
        } else if (table_counts) {
            uint64_t lwm = 0;
            if (matchy_scan_result_lines(&r, nullptr, nullptr, &lwm) == MATCHY_SUCCESS) t.lines_with_matches += lwm;
            else { fprintf(stderr, "[ERROR] no line context in a scan result: %s\n", matchy_amd_last_error()); d.ok = false; }
            if (line_ctx || !d.ok) return;   // the records of a scan with line numbers: render_numbered, in sequence order
        } else {
            // lines with matches: hits come sorted by offset; a new line starts when a '\n' lies between two hit starts (and a '\n' lies
            // between any two segments of a pack)
            size_t prev = (size_t)-1;
            for (size_t i = 0; i < r.n_hits; ++i) {
                const size_t s = (size_t)r.hits[i].start;
                if (prev == (size_t)-1 || memchr(data + prev, '\n', s - prev)) ++t.lines_with_matches;
                prev = s;
            }
        }
        if (json && r.n_hits && b.armed && take_gpu_text(r, d)) return;
        if (json && r.n_hits) {   // every match of the batch in one call (the scanner caches the rendered data payloads)
            char* text = nullptr;
            size_t n = 0;
            int32_t rc;
            if (!b.segmented()) rc = matchy_scan_result_to_ndjson(sc, &r, data, sources[b.input].c_str(), &text, &n);
            else { const std::vector<const char*> src = pack_sources(b); rc = matchy_scan_result_to_ndjson_segments(sc, &r, data, src.data(), nullptr, false, &text, &n); }
            if (rc == MATCHY_SUCCESS) { d.text = text; d.text_len = n; }
            else { fprintf(stderr, "[ERROR] rendering failed: %s\n", matchy_amd_last_error()); d.ok = false; }
        }
    }
    std::vector<const char*> pack_sources(const Batch& b) const {
        std::vector<const char*> src;   // one per segment
        b.each_input([&](size_t i) { src.push_back(sources[i].c_str()); });
        return src;
    }
    // the records of a batch of a scan with line context; `base` = lines of its input in front of it
    // (a packed input is whole: its lines count from zero)
    void render_numbered(matchy_scanner_t* sc, const matchy_scan_result_t& r, const uint8_t* data, const Batch& b, unsigned long long base, Done& d) {
        if (!json || !r.n_hits || !d.ok || d.skip) return;
        if (b.armed && take_gpu_text(r, d)) return;   // armed batches have base 0: a pack, or an input's first batch
        char* text = nullptr;
        size_t n = 0;
        int32_t rc;
        if (!b.segmented()) rc = matchy_scan_result_to_ndjson_lines(sc, &r, data, sources[b.input].c_str(), base, input_line, &text, &n);
        else {
            const std::vector<const char*> src = pack_sources(b);
            const std::vector<uint64_t> bases(src.size(), b.continues_lines() ? base : 0);   // a window goes on where the windows in front ended
            rc = matchy_scan_result_to_ndjson_segments(sc, &r, data, src.data(), bases.data(), input_line, &text, &n);
        }
        if (rc == MATCHY_SUCCESS) { d.text = text; d.text_len = n; }
        else { fprintf(stderr, "[ERROR] rendering failed: %s\n", matchy_amd_last_error()); d.ok = false; }
    }
    static void* batch_hook(void* user, size_t, matchy_scanner_t* sc, const matchy_scan_result_t* r, const uint8_t* data, size_t len, void* tag) {
        MatchPipeline* pl = (MatchPipeline*)user;
        Done* d = new Done();
        if (pl->whole_lines) pl->add_whole_lines(sc);
        if (((const Batch*)tag)->kind == BatchKind::UTF16) pl->add_utf16(sc, *r);
        if (((const Batch*)tag)->kind == BatchKind::ESCAPED) pl->add_unescaped(sc, *r, ((const Batch*)tag)->len);
        pl->render(sc, *r, data, len, *(const Batch*)tag, *d);
        return d;
    }
    // scan one batch on the calling thread and render its matches (--follow: one scanner, batches as they appear)
    void run_batch(matchy_scanner_t* sc, Batch& b, Done& d) {
        if (!b.len) return;
        matchy_scan_result_t r;
        memset(&r, 0, sizeof(r));
        if (matchy_scanner_scan(sc, b.ptr, b.len, &r) != MATCHY_SUCCESS) {
            fprintf(stderr, "[ERROR] scan failed: %s\n", matchy_amd_last_error());
            d.ok = false;
            return;
        }
        if (whole_lines) add_whole_lines(sc);
        render(sc, r, b.ptr, b.len, b, d);
        if (line_ctx) {   // --follow: batches of an input come one after the other, the count continues across the polls
            render_numbered(sc, r, b.ptr, b, line_base[b.input], d);
            line_base[b.input] += r.lines;
        }
        matchy_scan_result_free(&r);
    }
    // takes the batches back in sequence order and prints them, until the reader is done and nothing is pending
    void printer(Totals& total, std::vector<char>& input_failed) {
        for (;;) {
            matchy_multi_batch_t b;
            int32_t r = matchy_multi_scanner_next(ms, &b);
            if (r == 0) {
                if (!reader_done) { std::this_thread::sleep_for(std::chrono::microseconds(200)); continue; }   // between two submits
                r = matchy_multi_scanner_next(ms, &b);
                if (r == 0) return;
            }
            if (r != 1) { fprintf(stderr, "[ERROR] gathering results failed: %s\n", matchy_amd_last_error()); return; }
            Batch* hb = (Batch*)b.tag;
            Done* d = (Done*)b.payload;
            if (b.status != MATCHY_SUCCESS) {
                if (hb->is_gz()) hb->verdict->set(nullptr, 0);   // the pack was not scanned: the reader reads its files the old way
                else {
                    fprintf(stderr, "[ERROR] scan failed: %s\n", matchy_amd_last_error());
                    hb->each_input([&](size_t i) { input_failed[i] = 1; });
                }
            } else if (d) {
                if (line_ctx) {   // the worker's scanner renders here: with line context its hook renders nothing, so one thread at a time uses it
                    render_numbered(matchy_multi_scanner_worker_scanner(ms, b.worker), b.result, b.data, *hb, line_base[hb->input], *d);
                    if (hb->continues_lines()) line_base[hb->input] += b.result.lines;
                }
                if (!d->ok) hb->each_input([&](size_t i) { input_failed[i] = 1; });   // rendering failed: the batch's matches are missing, exit status says so
                if (d->text_len) write_all_stdout(d->text, d->text_len);
                total += d->t;
            }
            matchy_scan_result_free(&b.result);
            delete d;
            delete hb;   // frees an owned (read) batch's bytes; a mapped batch's pages go with its file's mapping
            release_mappings(b.seq + 1);
        }
    }
};

// Inputs ending in .gz (case-insensitive) are decompressed on the fly like the reference's file reader does
// (crates/matchy/src/file_reader.rs:45-75, by extension); "-" is stdin. Regular files are mapped and their batches are
// views of the mapping (no copy on the host; this thread pre-faults and pins each batch's pages ahead of its scan;
// MATCHY_AMD_NO_MMAP=1 reads them like a stream instead). Returns false when the input could not be read. Mappings are
// released by the printer as their files complete. skip (inputs that are read): the first `skip` bytes of the stream — what the gz windows
// in front have reported already (--gz-windows), which ends behind a '\n' — are read and cut into batches like the rest, so the cuts
// are those of the whole stream, but not submitted; 0 is the whole input.
// enc (--encoding): UTF16LE / UTF16BE read the input's byte stream — the mapped file, stdin, or what gzread returns — as UTF-16 in that
// byte order, AUTO does so when the stream begins with FF FE or FE FF and reads anything else as bytes. A leading BOM of the byte order
// in effect is skipped: it is not part of the text. The batches are cut behind 000A units (newline_cut16) and go out as they are.
// pl.unescape_modes (--unescape): the batches are cut as ever and go out as escaped ones.
bool read_input(MatchPipeline& pl, size_t input, const std::string& path, size_t batch_bytes, uint64_t skip = 0, Encoding enc = Encoding::BYTES) {
    const bool gz = ends_with_ci(path, ".gz");
    // the byte order for a stream that begins with b[0 .. n): -1 = bytes; `bom` = bytes of the BOM to skip
    auto utf16_order = [enc](const uint8_t* b, size_t n, size_t& bom) {
        bom = 0;
        const bool le = n >= 2 && b[0] == 0xFF && b[1] == 0xFE, be = n >= 2 && b[0] == 0xFE && b[1] == 0xFF;
        if (enc == Encoding::BYTES || (enc == Encoding::AUTO && !le && !be)) return -1;
        const int order = enc == Encoding::UTF16LE ? (int)MATCHY_UTF16_LE : enc == Encoding::UTF16BE ? (int)MATCHY_UTF16_BE : le ? (int)MATCHY_UTF16_LE : (int)MATCHY_UTF16_BE;
        if (order == (int)MATCHY_UTF16_LE ? le : be) bom = 2;
        return order;
    };
    int fd = path == "-" ? 0 : open(path.c_str(), O_RDONLY);
    if (fd < 0) { fprintf(stderr, "[ERROR] Failed to process %s: %s\n", path.c_str(), strerror(errno)); return false; }
    struct stat sb;
    if (!gz && fd != 0 && fstat(fd, &sb) == 0 && S_ISREG(sb.st_mode) && sb.st_size > 0 && !getenv("MATCHY_AMD_NO_MMAP")) {
        const size_t size = (size_t)sb.st_size;
        void* m = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
        if (m != MAP_FAILED) {
            close(fd);
            (void)madvise(m, size, MADV_SEQUENTIAL);
            size_t bom = 0;
            const int order = utf16_order((const uint8_t*)m, size, bom);
            if (order >= 0) ++pl.u16_inputs;
            const uint8_t* base = (const uint8_t*)m + bom;   // the first byte that is scanned (or transcoded: units lie at even offsets from it)
            const size_t text_size = size - bom;
            size_t last_seq = 0;
            for (size_t pos = 0; pos < text_size;) {
                const size_t end = order >= 0 ? newline_cut16(base, pos, text_size, batch_bytes, (uint32_t)order) : newline_cut(base, pos, text_size, batch_bytes);
                Batch b;
                if (order >= 0) { b.kind = BatchKind::UTF16; b.byte_order = (uint32_t)order; }
                else if (pl.unescape_modes) { b.kind = BatchKind::ESCAPED; b.unescape_modes = pl.unescape_modes; }
                b.input = input; b.ptr = base + pos; b.len = end - pos;
                b.reg = prefault_and_pin(b.ptr, b.len);
                last_seq = pl.submit(std::move(b));
                pos = end;
            }
            pl.add_mapping(m, size, last_seq);
            if (input < pl.consumed.size()) pl.consumed[input] = (long long)size;
            return true;
        }
    }
    gzFile zf = nullptr;
    if (gz) {
        zf = gzdopen(fd, "rb");
        if (!zf) { fprintf(stderr, "[ERROR] Failed to process %s: cannot start gzip decoder\n", path.c_str()); close(fd); return false; }
        gzbuffer(zf, 1u << 20);
    }
    size_t total_read = 0;
    auto rd_raw = [&](void* p, size_t n) {
        const ssize_t r = gz ? (ssize_t)gzread(zf, p, (unsigned)n) : read(fd, p, n);
        if (r < 0 && gz) errno = EIO;   // the decoder keeps its error: a retry would fail again
        return r;
    };
    // --encoding: the stream's first two bytes are read ahead; what is no BOM to skip is handed to the batch reader first
    uint8_t head[2];
    size_t n_head = 0, head_pos = 0;
    int order = -1;
    bool head_failed = false;
    if (enc != Encoding::BYTES) {
        while (n_head < 2) {
            const ssize_t r = rd_raw(head + n_head, 2 - n_head);
            if (r < 0) { if (errno == EINTR) continue; head_failed = true; break; }
            if (r == 0) break;
            n_head += (size_t)r;
        }
        size_t bom = 0;
        order = utf16_order(head, n_head, bom);
        head_pos = bom;
        if (order >= 0) ++pl.u16_inputs;
    }
    auto rd = [&](void* p, size_t n) -> ssize_t {
        if (head_pos < n_head) { const size_t k = std::min(n, n_head - head_pos); memcpy(p, head + head_pos, k); head_pos += k; return (ssize_t)k; }
        return rd_raw(p, n);
    };
    auto sink = [&](Bytes&& data, size_t len, uint64_t off) {
        total_read += len;
        if (off + len <= skip) return true;   // reported already
        const size_t drop = off < skip ? (size_t)(skip - off) : 0;   // skip lies behind a '\n': what is left starts a line
        Batch b;
        if (order >= 0) { b.kind = BatchKind::UTF16; b.byte_order = (uint32_t)order; }
        else if (pl.unescape_modes) { b.kind = BatchKind::ESCAPED; b.unescape_modes = pl.unescape_modes; }
        b.input = input; b.ptr = data.get() + drop; b.len = len - drop; b.own = std::move(data);
        pl.submit(std::move(b));
        return true;
    };
    const StreamEnd e = head_failed ? StreamEnd::FAILED : order >= 0 ? read_batches16(rd, batch_bytes, (uint32_t)order, sink) : read_batches(rd, batch_bytes, sink);
    const bool ok = e == StreamEnd::DONE;
    if (!ok) { int ze; fprintf(stderr, "[ERROR] Failed to process %s: %s\n", path.c_str(), gz && errno == EIO ? gzerror(zf, &ze) : strerror(errno)); }
    if (gz) gzclose(zf);   // closes fd as well
    else if (fd) close(fd);
    if (ok && !gz && fd != 0 && input < pl.consumed.size()) pl.consumed[input] = (long long)total_read;
    return ok;
}

// -f / --follow (match_processor/follow.rs:20-264): after the existing content, keep watching the files and scan what is
// appended — from the last known size to the new one, whatever it ends with, as the reference's `reader.lines()` does; a
// file that shrank is read again from the start; a file that disappeared is reported once. Records carry the wall-clock
// time of their batch as `timestamp` (the parallel path's constant "0.000" everywhere else). Ends on SIGINT / SIGTERM.
volatile sig_atomic_t g_stop = 0;
void on_stop(int) { g_stop = 1; }

void follow_inputs(MatchPipeline& pl, matchy_scanner_t* sc, const std::vector<std::string>& paths, bool stats, Totals& total) {
    struct Tail { std::string path; size_t input; off_t pos; bool gone; };
    std::vector<Tail> tails;
    for (size_t i = 0; i < paths.size(); ++i) {
        struct stat sb;
        // from where the first pass stopped reading; inputs it could not count (.gz, unreadable): from their size now
        const bool counted = i < pl.consumed.size() && pl.consumed[i] >= 0;
        tails.push_back({paths[i], i, counted ? (off_t)pl.consumed[i] : (stat(paths[i].c_str(), &sb) == 0 ? sb.st_size : 0), false});
    }
    struct sigaction sa;
    memset(&sa, 0, sizeof(sa));
    sa.sa_handler = on_stop;
    sigaction(SIGINT, &sa, nullptr);
    sigaction(SIGTERM, &sa, nullptr);
    if (stats) fprintf(stderr, "[INFO] Watching for new content (Ctrl+C to stop)...\n");
    while (!g_stop) {
        bool any = false;
        for (Tail& tl : tails) {
            struct stat sb;
            if (stat(tl.path.c_str(), &sb) != 0) {
                if (!tl.gone && stats) fprintf(stderr, "[WARN] File deleted/rotated: %s\n", tl.path.c_str());
                tl.gone = true;
                continue;
            }
            tl.gone = false;
            if (sb.st_size < tl.pos) { tl.pos = 0; if (tl.input < pl.line_base.size()) pl.line_base[tl.input] = 0; }   // truncated: start over
            if (sb.st_size == tl.pos) continue;
            const int fd = open(tl.path.c_str(), O_RDONLY);
            if (fd < 0) continue;
            Batch b;
            b.input = tl.input;
            b.own.reset((uint8_t*)malloc((size_t)(sb.st_size - tl.pos) + 16));
            if (!b.own) { close(fd); continue; }
            size_t have = 0;
            while (have < (size_t)(sb.st_size - tl.pos)) {
                const ssize_t n = pread(fd, b.own.get() + have, (size_t)(sb.st_size - tl.pos) - have, tl.pos + (off_t)have);
                if (n <= 0) break;
                have += (size_t)n;
            }
            close(fd);
            tl.pos += (off_t)have;
            if (!have) continue;
            any = true;
            b.ptr = b.own.get(); b.len = have;
            Done d;
            pl.run_batch(sc, b, d);
            if (d.text_len) d.out.assign(d.text, d.text_len);
            if (!d.out.empty()) {
                // this batch's records carry the current time
                char ts[48];
                struct timespec now;
                clock_gettime(CLOCK_REALTIME, &now);
                snprintf(ts, sizeof(ts), "\"timestamp\":\"%.3f\"}", (double)now.tv_sec + (double)now.tv_nsec * 1e-9);
                static const std::string fixed = "\"timestamp\":\"0.000\"}";
                std::string out;
                size_t from = 0;
                for (;;) {
                    const size_t k = d.out.find(fixed + "\n", from);
                    if (k == std::string::npos) { out.append(d.out, from, std::string::npos); break; }
                    out.append(d.out, from, k - from);
                    out += ts;
                    from = k + fixed.size();
                }
                fwrite(out.data(), 1, out.size(), stdout);
                fflush(stdout);
            }
            total += d.t;
        }
        if (!any) usleep(100 * 1000);
    }
    if (stats) fprintf(stderr, "[INFO] Follow mode stopped\n");
}

// Inputs read the way they are read without any flag; `failed` is the reader thread's list (input_failed is the printer's until it is joined).
struct HostReader {
    MatchPipeline& pl;
    const std::vector<std::string>& paths;
    size_t batch_bytes;
    std::vector<char> failed;
    Encoding encoding = Encoding::BYTES;   // --encoding
    // bytes: the gz side's batches stay below 2^31
    void read(size_t i, uint64_t skip = 0, size_t bytes = 0) { if (!read_input(pl, i, paths[i], bytes ? bytes : batch_bytes, skip, encoding)) failed[i] = 1; }
};

// --gz-on-gpu, the reader's side. Which .gz input goes into the pack in hand and when a pack goes out is decided by the packer
// (gz_packer.h); this is what waits. Before anything else is submitted, barrier() sends the pack in hand and waits for the verdict on
// it: the files the GPU did not accept are read the old way there, right behind their pack, so the order of everything else is that of
// the command line. While a pack is on the GPU the reader goes on reading files for the next.
struct GzReader {
    MatchPipeline& pl;
    HostReader& host;
    GzPacker packer;
    std::shared_ptr<GzVerdict> pending;
    std::vector<GzFile> pending_files;
    size_t on_gpu = 0, packs = 0, on_host = 0;
    unsigned long long packed_bytes = 0, text_bytes = 0;
    size_t multi_files = 0, multi_members = 0;   // --gz-members, of the files the GPU accepted: those of more than one member, and their members
    // --gz-windows: a multi-member .gz input that the packer leaves (larger than a batch, or more text than a pack holds) is mapped and
    // goes out as a chain of windows of whole members: up to max_text of text and batch_bytes compressed each.
    bool windows = false;
    size_t win_windows = 0, win_files = 0, win_host = 0;   // windows the GPU accepted, files that went out as windows, of those finished on the host
    // --gz-stream-windows: a .gz input of ONE member that the packer leaves (compressed or inflated, it does not fit a pack) is mapped and
    // goes out as a chain of stream windows (gz_stream.h): up to stream_text_cap of text each, in pieces of piece_bytes.
    bool stream_windows = false;
    uint32_t piece_bytes = 0;
    size_t sw_windows = 0, sw_files = 0, sw_host = 0;      // the same three counts for stream windows

    GzReader(MatchPipeline& p, HostReader& h, bool members, bool win, uint32_t pieces, bool stream_win) : pl(p), host(h), windows(win), stream_windows(stream_win), piece_bytes(pieces) {
        auto env = [](const char* name) { const char* e = getenv(name); return e ? std::optional<uint64_t>(strtoull(e, nullptr, 10)) : std::nullopt; };
        // --gz-pieces: a member is inflated by many waves, so it may be as large as a pack holds
        packer.bounds = (pieces ? gz_bounds_pieces : gz_bounds)(h.batch_bytes, env("MATCHY_AMD_GZ_MAX_MEMBER"), env("MATCHY_AMD_GZ_MAX_CARRY"));
        packer.members = members;
        packer.on_pack = [this](const std::vector<uint8_t>& packed, const std::vector<GzFile>& files) { send(packed, files); };
        // behind the pack in hand and its verdict: as a chain of windows, or the way it is read without the flags
        packer.not_eligible = [this](size_t i) { settle(); if (!take_windows(i) && !take_stream_windows(i)) host.read(i); };
    }
    void take(size_t i) { packer.take(i, host.paths[i]); }
    void barrier() { packer.flush(); settle(); }
    // --gz-windows, behind barrier(): input i as a chain of windows. False: not eligible (no regular .gz file, a first header that does
    // not parse, a first member that alone breaks a bound), nothing was submitted and the input is read the way it is without the flag.
    // The windows go out one at a time: the reader waits for a window's verdict, and with it the carry, before it submits the next —
    // and faults the next window's pages in meanwhile. A window the GPU does not accept (a member that fails, NO_LINE_END, a scan that
    // failed) or a member the walker cannot take ends the chain: everything reported so far is right — verified members, complete
    // lines only — and the host reads the file the way it does without the flag and reports what lies behind the bytes the accepted
    // windows consumed. A file whose decoder fails loses the batch the host was filling, as it does without the flag: the records are
    // those of the run without the flag, plus — where the windows had got further than the host's last batch cut — the complete lines
    // in between.
    bool take_windows(size_t i) {
        const std::string& path = host.paths[i];
        const GzBounds& bd = packer.bounds;
        struct stat sb;
        if (!windows || !pack_ends_with_gz(path)) return false;
        const int fd = open(path.c_str(), O_RDONLY);
        if (fd < 0) return false;
        if (fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode) || sb.st_size < 18) { close(fd); return false; }
        const size_t size = (size_t)sb.st_size;
        void* m = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
        close(fd);
        if (m == MAP_FAILED) return false;
        const uint8_t* p = (const uint8_t*)m;
        GzWindow cur, nxt;
        if (!gz_next_window(p, size, 0, bd.batch_bytes, bd.max_text, bd.max_member, cur)) { munmap(m, size); return false; }
        ++win_files;
        std::vector<uint8_t> carry;
        uint64_t from = 0, consumed = 0;
        size_t last_seq = 0;
        bool ok = false;
        for (;;) {
            Batch b;
            b.kind = BatchKind::GZ_WINDOW; b.input = i; b.ptr = p + from; b.len = (size_t)(cur.end - from);
            b.window_last = cur.end == size; b.carry = carry; b.carry_cap = (uint32_t)bd.carry_cap;
            b.gz.push_back(GzFile{i, 0, (uint32_t)b.len, (uint32_t)cur.text, cur.members});
            b.verdict = std::make_shared<GzVerdict>();
            const std::shared_ptr<GzVerdict> v = b.verdict;
            last_seq = pl.submit(std::move(b));
            const bool have_next = cur.end < size && gz_next_window(p, size, cur.end, bd.batch_bytes, bd.max_text, bd.max_member, nxt);
            if (have_next) { volatile uint8_t sink = 0; for (uint64_t q = cur.end; q < nxt.end; q += 4096) sink = sink + p[q]; }
            v->wait();
            if (v->status.size() != 1 || v->status[0] != MATCHY_GZ_OK || v->window_status != MATCHY_WINDOW_OK) break;
            ++win_windows; consumed += v->bytes;
            carry = std::move(v->carry);
            if (cur.end == size) { ok = true; break; }
            if (!have_next) break;   // the next member alone breaks a bound
            from = cur.end; cur = nxt;
        }
        pl.add_mapping(m, size, last_seq);
        if (!ok) { ++win_host; host.read(i, consumed, bd.batch_bytes); }
        return true;
    }
    // --gz-stream-windows, behind barrier() and take_windows(): input i as a chain of stream windows. False: not eligible (no regular .gz
    // file, a header that does not parse, more than one member), nothing was submitted. The walker of gz_stream.h says where a window
    // starts and how many bytes it gets; the windows go out one at a time, each with the state and the carry of the one in front, and the
    // reader faults the next window's pages in while it waits. A window that is not OK ends the chain: what the windows in front
    // reported is right — complete lines of text whose every block parsed — and the host finishes the file from the bytes they
    // consumed, as for --gz-windows. The trailer is verified in the last window: a file whose CRC or length is wrong has had its text
    // reported by then, the [ERROR] line is the host's.
    bool take_stream_windows(size_t i) {
        const std::string& path = host.paths[i];
        const GzBounds& bd = packer.bounds;
        struct stat sb;
        if (!stream_windows || !piece_bytes || !pack_ends_with_gz(path) || bd.max_text < 2) return false;
        const int fd = open(path.c_str(), O_RDONLY);
        if (fd < 0) return false;
        if (fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode) || sb.st_size < 18) { close(fd); return false; }
        const size_t size = (size_t)sb.st_size;
        void* m = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
        close(fd);
        if (m == MAP_FAILED) return false;
        const uint8_t* p = (const uint8_t*)m;
        uint64_t body = 0, next = 0, next_body = 0;
        if (gz_parse_header(p, size, body) != GZ_PLAN_OK || size - body < 8 || gz_next_member(p, size, 0, body, next, next_body)) { munmap(m, size); return false; }
        // carry + text + the separator fit a batch; a window's compressed bytes are no more than its text may be
        const uint32_t text_cap = (uint32_t)std::min<uint64_t>(bd.max_text - 1, 0x7FF00000ull - bd.carry_cap);
        const uint32_t window_bytes = (uint32_t)std::max<uint64_t>(std::min<uint64_t>(bd.batch_bytes, text_cap), piece_bytes);
        GzStreamWalker walk(size, window_bytes, piece_bytes, text_cap, window_bytes / 4);
        ++sw_files;
        std::vector<uint8_t> carry;
        std::shared_ptr<matchy_gz_stream_state_t> state;
        uint64_t consumed = 0;
        size_t last_seq = 0;
        while (!walk.over) {
            const GzStreamWindow w = walk.next();
            Batch b;
            b.kind = BatchKind::GZ_STREAM; b.input = i; b.ptr = p + w.offset; b.len = (size_t)w.len;
            b.carry = carry; b.carry_cap = (uint32_t)bd.carry_cap; b.stream_state = state; b.stream_text_cap = text_cap; b.stream_flags = w.flags;
            b.gz.push_back(GzFile{i, 0, (uint32_t)b.len, 0, 1});
            b.verdict = std::make_shared<GzVerdict>();
            const std::shared_ptr<GzVerdict> v = b.verdict;
            last_seq = pl.submit(std::move(b));
            { volatile uint8_t sink = 0; for (uint64_t q = w.offset + w.len, end = std::min<uint64_t>(size, q + w.len); q < end; q += 4096) sink = sink + p[q]; }
            v->wait();
            if (v->status.size() != 1 || v->stream_status != MATCHY_STREAM_OK || !v->state) { walk.refuse(); break; }
            if (!walk.accept(w, v->consumed_bits, v->text_len, v->ended)) break;
            ++sw_windows; consumed += v->bytes;
            carry = std::move(v->carry); state = v->state;
        }
        pl.add_mapping(m, size, last_seq);
        if (!walk.ended) { ++sw_host; host.read(i, consumed, bd.batch_bytes); }
        return true;
    }
    // the verdict on the pack that is out: what the GPU accepted is counted, the rest is read the old way now
    void settle() {
        if (!pending) return;
        pending->wait();
        for (size_t k = 0; k < pending_files.size(); ++k) {
            const GzFile& g = pending_files[k];
            if (k < pending->status.size() && pending->status[k] == MATCHY_GZ_OK) {
                ++on_gpu; packed_bytes += g.len; text_bytes += g.isize;
                if (g.members > 1) { ++multi_files; multi_members += g.members; }
                continue;
            }
            ++on_host;
            host.read(g.input, 0, packer.bounds.batch_bytes);
        }
        pending.reset();
        pending_files.clear();
    }
    // a pack the packer has completed goes out, behind the verdict on the one in front of it
    void send(const std::vector<uint8_t>& packed, const std::vector<GzFile>& files) {
        settle();
        Batch b;
        b.own.reset((uint8_t*)malloc(packed.size()));
        if (!b.own) {   // no memory for the pack: its files go the old way
            for (const GzFile& g : files) { ++on_host; host.read(g.input, 0, packer.bounds.batch_bytes); }
            return;
        }
        memcpy(b.own.get(), packed.data(), packed.size());
        b.kind = BatchKind::GZ_PACK; b.input = files[0].input; b.ptr = b.own.get(); b.len = packed.size();
        b.gz = files; b.verdict = std::make_shared<GzVerdict>();
        pending = b.verdict; pending_files = files;
        ++packs;
        pl.submit(std::move(b));
    }
};

struct MatchOptions {
    std::vector<std::string> pos;   // the database, then the inputs
    std::string format = "json", extractors, devices;
    bool stats = false, follow = false, line_numbers = false, input_line = false, tally = false, pack = false, gz_gpu = false, gz_members = false, gz_windows = false, gz_stream_windows = false, gather_lines = false, render_gpu = false, whole_lines = false;
    size_t tally_limit = 20;   // --tally[=N]: rows of the report, 0 = all
    // --encoding=utf-16le|utf-16be|auto: UTF-16 inputs are transcoded on the GPU in front of the scan; `encoding_given`: the flag was there
    Encoding encoding = Encoding::BYTES;
    bool encoding_given = false;
    // --unescape=percent|json|json+percent: the batches are decoded on the GPU in front of the scan (MATCHY_UNESCAPE_*; 0: off)
    uint32_t unescape_modes = 0;
    // --gz-pieces[=BYTES] (with --gz-on-gpu): one large DEFLATE stream is inflated by many waves, in pieces of BYTES compressed bytes; 0 = off.
    // The default is the best of the sweep of tools/gz_pieces_timing.py: 4, 8 and 16 KiB lie within 3 % of each other on
    // level 6 log text, whose blocks have about 32 KiB; from 32 KiB on a piece holds more than one block and the time doubles.
    uint32_t gz_pieces = 0;
    static constexpr uint32_t GZ_PIECES_DEFAULT = 8192;
    size_t batch_bytes = (size_t)256 << 20;  // GPU batches: large, so that one launch amortises PCIe latency
    int device = 0;
    int jobs = 0;   // -j N|auto (matchy.rs:98-103: worker threads): scanners here; auto = 2 (summary) / 4 (json) per device listed once
};

// the command line into `o`; -1, or the exit status of a command line that cannot be run
int parse_match_options(int argc, char** argv, MatchOptions& o) {
    typedef MatchOptions M;
    static const struct { const char* name; bool M::*on; } switches[] = {
        {"-s", &M::stats}, {"--stats", &M::stats}, {"-f", &M::follow}, {"--follow", &M::follow}, {"--line-numbers", &M::line_numbers}, {"--input-line", &M::input_line},
        {"--pack-inputs", &M::pack}, {"--gz-on-gpu", &M::gz_gpu}, {"--gz-members", &M::gz_members}, {"--gz-windows", &M::gz_windows}, {"--gz-stream-windows", &M::gz_stream_windows}, {"--gather-lines", &M::gather_lines},
        {"--render-on-gpu", &M::render_gpu}, {"--whole-lines", &M::whole_lines}, {"--tally", &M::tally}};
    if (const char* d = getenv("MATCHY_AMD_DEVICE")) o.device = atoi(d);
    for (int i = 0; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&](const char* name) -> const char* { if (i + 1 >= argc) { fprintf(stderr, "error: %s needs a value\n", name); exit(2); } return argv[++i]; };
        auto eqval = [&](const char* name, std::string& out) {  // --name=value or --name value
            size_t n = strlen(name);
            if (a.compare(0, n, name) != 0) return false;
            if (a.size() == n) { out = next(name); return true; }
            if (a[n] == '=') { out = a.substr(n + 1); return true; }
            return false;
        };
        std::string v;
        bool is_switch = false;
        for (const auto& s : switches) if (a == s.name) { o.*s.on = true; is_switch = true; }
        if (is_switch) continue;
        if (eqval("--format", v)) o.format = v;
        else if (eqval("--encoding", v)) {
            o.encoding_given = true;
            if (v == "utf-16le") o.encoding = Encoding::UTF16LE;
            else if (v == "utf-16be") o.encoding = Encoding::UTF16BE;
            else if (v == "auto") o.encoding = Encoding::AUTO;
            else { fprintf(stderr, "Error: Unknown encoding: %s. Use 'utf-16le', 'utf-16be' or 'auto'\n", v.c_str()); return 1; }
        }
        else if (eqval("--batch-bytes", v)) { size_t b = strtoull(v.c_str(), nullptr, 10); if (b >= 4096) o.batch_bytes = b; }
        else if (eqval("--extractors", v)) o.extractors = v;
        else if (eqval("--devices", v)) o.devices = v;
        else if (eqval("--device", v)) o.device = atoi(v.c_str());
        else if (eqval("--threads", v) || eqval("--readers", v) || eqval("--cache-size", v)) {}
        else if (a == "-j") { const std::string j = next("-j"); o.jobs = j == "auto" ? 0 : std::max(0, atoi(j.c_str())); }
        else if (a == "-p" || a == "--progress" || a == "--debug-routing") {}
        else if (a.compare(0, 8, "--tally=") == 0) {
            const std::string n = a.substr(8);
            if (n.empty() || n.find_first_not_of("0123456789") != std::string::npos) { fprintf(stderr, "error: --tally=N needs a number, got '%s'\n", n.c_str()); return 2; }
            o.tally = true; o.tally_limit = strtoull(n.c_str(), nullptr, 10);
        }
        else if (a == "--gz-pieces") o.gz_pieces = M::GZ_PIECES_DEFAULT;
        else if (a.compare(0, 12, "--gz-pieces=") == 0) {
            const std::string n = a.substr(12);
            const unsigned long long b = n.empty() || n.find_first_not_of("0123456789") != std::string::npos ? 0ull : strtoull(n.c_str(), nullptr, 10);
            if (b > 0xFFFFFFFFull || !gz_piece_bytes_valid((uint32_t)b)) { fprintf(stderr, "error: --gz-pieces=BYTES needs a power of two from 512 to 1048576, got '%s'\n", n.c_str()); return 2; }
            o.gz_pieces = (uint32_t)b;
        }
        else if (eqval("--unescape", v)) {
            if (v == "percent") o.unescape_modes = MATCHY_UNESCAPE_PERCENT;
            else if (v == "json") o.unescape_modes = MATCHY_UNESCAPE_JSON;
            else if (v == "json+percent") o.unescape_modes = MATCHY_UNESCAPE_JSON | MATCHY_UNESCAPE_PERCENT;
            else { fprintf(stderr, "Error: Unknown escape grammar: %s. Use 'percent', 'json' or 'json+percent'\n", v.c_str()); return 1; }
        }
        else if (a.size() > 1 && a[0] == '-') { fprintf(stderr, "error: unexpected argument '%s'\n", a.c_str()); return 2; }
        else o.pos.push_back(a);
    }
    if (o.pos.size() < 2) return usage();
    auto refuse = [](const char* why) { fprintf(stderr, "Error: %s\n", why); return 1; };
    if (o.format != "json" && o.format != "summary") { fprintf(stderr, "Error: Unknown format: %s. Use 'json' or 'summary'\n", o.format.c_str()); return 1; }
    if (o.encoding_given) {
        // the batches of a UTF-16 input are transcoded whole, on the GPU, in front of a plain scan: no segments, no compressed bytes, no queries
        if (o.follow) return refuse("--encoding is not supported with --follow (a followed file is read as bytes as it grows)");
        if (o.pack) return refuse("--encoding is not supported with --pack-inputs (a UTF-16 batch has no segments)");
        if (o.gz_gpu) return refuse("--encoding is not supported with --gz-on-gpu (the GPU inflates .gz inputs into UTF-8 text; without the flag they are inflated on the host and transcoded)");
        if (o.gz_members) return refuse("--encoding is not supported with --gz-members (it extends --gz-on-gpu)");
        if (o.gz_windows) return refuse("--encoding is not supported with --gz-windows (it extends --gz-on-gpu)");
        if (o.gz_stream_windows) return refuse("--encoding is not supported with --gz-stream-windows (it extends --gz-on-gpu)");
        if (o.gz_pieces) return refuse("--encoding is not supported with --gz-pieces (it extends --gz-on-gpu)");
        if (o.whole_lines) return refuse("--encoding is not supported with --whole-lines (whole-line queries read their input as bytes)");
    }
    if (o.unescape_modes) {
        // the batches of an input are decoded whole, on the GPU, in front of a plain scan: no segments, no compressed bytes, no queries
        if (o.follow) return refuse("--unescape is not supported with --follow (a followed file is scanned as it grows, as it is)");
        if (o.pack) return refuse("--unescape is not supported with --pack-inputs (a decoded batch has no segments)");
        if (o.gz_gpu) return refuse("--unescape is not supported with --gz-on-gpu (the GPU inflates .gz inputs into the text that is scanned; without the flag they are inflated on the host and decoded)");
        if (o.gz_members) return refuse("--unescape is not supported with --gz-members (it extends --gz-on-gpu)");
        if (o.gz_windows) return refuse("--unescape is not supported with --gz-windows (it extends --gz-on-gpu)");
        if (o.gz_stream_windows) return refuse("--unescape is not supported with --gz-stream-windows (it extends --gz-on-gpu)");
        if (o.gz_pieces) return refuse("--unescape is not supported with --gz-pieces (it extends --gz-on-gpu)");
        if (o.whole_lines) return refuse("--unescape is not supported with --whole-lines (whole-line queries read their input as it is)");
        if (o.encoding_given) return refuse("--unescape is not supported with --encoding (one front pass per batch: transcode the input first)");
    }
    if (o.gz_windows && !(o.gz_gpu && o.gz_members)) return refuse("--gz-windows needs --gz-on-gpu --gz-members (it extends them to multi-member files larger than a batch)");
    if (o.gz_stream_windows && !(o.gz_gpu && o.gz_pieces)) return refuse("--gz-stream-windows needs --gz-on-gpu --gz-pieces (it extends them to one DEFLATE stream larger than a batch)");
    if (o.gz_members && !o.gz_gpu) return refuse("--gz-members needs --gz-on-gpu (it extends the gz packs to files of many members)");
    if (o.gz_pieces && !o.gz_gpu) return refuse("--gz-pieces needs --gz-on-gpu (it inflates one large stream of a gz pack with many waves)");
    if (o.whole_lines) {
        // the mode has no extraction to configure, and the library refuses it together with segments, gz scans, hit lines and rendered records
        const char* other = !o.extractors.empty() ? "--extractors" : o.pack ? "--pack-inputs" : o.gz_gpu ? "--gz-on-gpu" : o.gz_pieces ? "--gz-pieces" : o.gather_lines ? "--gather-lines" : o.render_gpu ? "--render-on-gpu" : nullptr;
        if (other) { fprintf(stderr, "Error: --whole-lines is not supported with %s\n", other); return 1; }
    }
    if (o.follow && o.tally) return refuse("--tally is not supported with --follow (the report is printed after the last batch)");
    if (o.follow && o.pack) return refuse("--pack-inputs is not supported with --follow (a followed file grows; a packed one is whole)");
    if (o.follow && o.render_gpu) return refuse("--render-on-gpu is not supported with --follow (a followed file's batches continue a line count only the printer knows)");
    if (o.follow && o.gz_gpu) return refuse("--gz-on-gpu is not supported with --follow (a followed file grows; a gz pack is whole)");
    if (o.follow && o.stats) fprintf(stderr, "[INFO] Processing existing file content...\n");
    if (o.follow) for (size_t i = 1; i < o.pos.size(); ++i) if (o.pos[i] == "-") return refuse("--follow mode not supported with stdin");
    return -1;
}

// device list: one worker (scanner) per entry; an entry may repeat (two scanners on one GPU overlap one batch's transfers with the
// other's kernels). False: the list cannot be used (said on stderr).
bool expand_devices(const MatchOptions& o, std::vector<int>& devs) {
    if (o.devices.empty()) devs.push_back(o.device);
    else if (o.devices == "all") {
        const int n = matchy_amd_device_count();
        if (n < 1) { fprintf(stderr, "Error: no HIP device available\n"); return false; }
        for (int d = 0; d < n; ++d) devs.push_back(d);
    } else {
        std::stringstream ss(o.devices);
        std::string part;
        while (std::getline(ss, part, ',')) {
            part = trim(part);
            if (part.empty() || part.find_first_not_of("0123456789") != std::string::npos) { fprintf(stderr, "Error: bad --devices entry '%s'\n", part.c_str()); return false; }
            devs.push_back(atoi(part.c_str()));
        }
        if (devs.empty()) { fprintf(stderr, "Error: --devices needs at least one device\n"); return false; }
    }
    // Workers. A device that is listed once gets several scanners (-j N: N in all, spread over the devices): one scanner's hit
    // post-processing runs under another's transfer (one scanner per GPU: 24 GB/s in the scan phase, two: 44). A device list
    // with repeats is taken as written.
    std::vector<int> uniq = devs;
    std::sort(uniq.begin(), uniq.end());
    if (std::adjacent_find(uniq.begin(), uniq.end()) != uniq.end()) return true;
    // auto: two scanners per device keep the bus busy when only counters come back (one copies while the other post-processes);
    // rendering NDJSON is per-hit host work, which four workers share better
    const size_t want = o.jobs > 0 ? std::max<size_t>((size_t)o.jobs, devs.size()) : devs.size() * (o.format == "json" ? 4 : 2);
    const std::vector<int> base = devs;
    for (size_t k = base.size(); k < want; ++k) devs.push_back(base[k % base.size()]);
    return true;
}

// database: .mxy file, or a .csv / .json source that is built in memory first (match_cmd.rs:20-31, 222-239)
matchy_t* open_database(const std::string& dbpath) {
    matchy_t* db = nullptr;
    if (ends_with_ci(dbpath, ".csv") || ends_with_ci(dbpath, ".json")) {
        DatabaseBuilder b;
        std::string err;
        std::vector<uint8_t> blob;
        if (!add_inputs(b, {dbpath}, ends_with_ci(dbpath, ".csv") ? "csv" : "json", false, err) || !b.build(blob)) {
            fprintf(stderr, "Error: %s\n", err.empty() ? b.error().c_str() : err.c_str());
            return nullptr;
        }
        db = matchy_open_buffer(blob.data(), blob.size());
    } else db = matchy_open(dbpath.c_str());
    if (!db) fprintf(stderr, "Error: Failed to open database %s: %s\n", dbpath.c_str(), matchy_amd_last_error());
    return db;
}

// The reader: every input in the order of the command line — into a plain pack, into the gz pack in hand, or the way it is read
// without the flags — while the printer thread takes the batches back. Returns when the last batch has been printed.
void run_inputs(const MatchOptions& o, MatchPipeline& pl, HostReader& host, GzReader& gzr, PackStats& packed, Totals& t, std::vector<char>& input_failed) {
    const std::vector<std::string>& paths = host.paths;
    std::thread printer([&] { pl.printer(t, input_failed); });
    auto single = [&](size_t i) { if (o.gz_gpu) gzr.take(i); else host.read(i); };   // an input that is not part of a plain pack
    if (o.pack) {
        // runs of small files go out as packs, everything else the way it goes without the flag, in the order of the command line
        packed = pack_inputs(
            paths, o.batch_bytes,
            [&](InputPack&& p) {
                if (o.gz_gpu) gzr.barrier();
                Batch b;
                b.kind = BatchKind::PACK; b.input = p.inputs[0].input; b.ptr = p.data.get(); b.len = p.len; b.own = std::move(p.data);
                b.pack = std::move(p.inputs); b.appended = p.appended;
                b.reg = prefault_and_pin(b.ptr, b.len);
                pl.submit(std::move(b));
            },
            single,
            [&](size_t i, int err) { fprintf(stderr, "[ERROR] Failed to process %s: %s\n", paths[i].c_str(), strerror(err)); host.failed[i] = 1; });
    } else for (size_t i = 0; i < paths.size(); ++i) single(i);
    if (o.gz_gpu) gzr.barrier();
    pl.reader_done = true;
    printer.join();
    for (size_t i = 0; i < paths.size(); ++i) if (host.failed[i]) input_failed[i] = 1;
    for (size_t i : pl.rejected_inputs) if (i < input_failed.size()) input_failed[i] = 1;
}

// --tally: the workers' tables merged, one JSON line per distinct matched value behind the match records; what the database holds for
// a value is asked of it now (a host query per row of the report). False: the tally could not be read.
bool report_tally(matchy_multi_scanner_t* ms, matchy_t* db, size_t limit, uint64_t& distinct) {
    matchy_tally_t tl;
    if (matchy_multi_scanner_tally_top(ms, limit, &tl) != MATCHY_SUCCESS) {
        fprintf(stderr, "Error: Failed to read the hit tally: %s\n", matchy_amd_last_error());
        return false;
    }
    distinct = tl.distinct;
    std::string line;
    for (size_t i = 0; i < tl.n_entries; ++i) {
        const matchy_tally_entry_t& e = tl.entries[i];
        const std::string text((const char*)e.text, e.len);
        line = "{\"count\":" + std::to_string((unsigned long long)e.count) + ",\"item_type\":";
        json_escape(matchy_item_type_name(e.item_type), line);
        line += ",\"matched_text\":";
        json_escape(text, line);
        line += ",\"result\":";
        int32_t found = 0;
        char* js = matchy_amd_query_json(db, text.c_str(), &found);
        line += js ? js : "[]";
        if (js) matchy_free_string(js);
        line += "}\n";
        fwrite(line.data(), 1, line.size(), stdout);
    }
    matchy_tally_free(&tl);
    return true;
}

// -s: the [INFO] statistics block (commands/match_cmd.rs:514-581), then what this build adds about its devices and modes
void report_stats(const MatchOptions& o, const MatchPipeline& pl, const GzReader& gzr, const PackStats& packed, const Totals& t, const std::vector<int>& devs,
                  size_t processed, size_t failed, double secs, const uint64_t* tally_distinct) {
    fprintf(stderr, "\n[INFO] === Processing Complete ===\n");
    if (o.pos.size() > 2) {
        fprintf(stderr, "[INFO] Files processed: %zu\n", processed);
        if (failed) fprintf(stderr, "[INFO] Files failed: %zu\n", failed);
    }
    fprintf(stderr, "[INFO] Lines processed: %s\n", fmt_num(t.lines).c_str());
    fprintf(stderr, "[INFO] Lines with matches: %s (%.1f%%)\n", fmt_num(t.lines_with_matches).c_str(),
            t.lines ? 100.0 * (double)t.lines_with_matches / (double)t.lines : 0.0);
    fprintf(stderr, "[INFO] Total matches: %s\n", fmt_num(t.matches).c_str());
    fprintf(stderr, "[INFO] Candidates tested: %s\n", fmt_num(t.candidates).c_str());
    if (o.whole_lines) fprintf(stderr, "[INFO] Whole-line queries: %s (%s addresses, %s strings, %s not valid UTF-8)\n", fmt_num(pl.wl_counters[0].load()).c_str(),
                               fmt_num(pl.wl_counters[1].load()).c_str(), fmt_num(pl.wl_counters[2].load()).c_str(), fmt_num(pl.wl_counters[3].load()).c_str());
    if (tally_distinct) fprintf(stderr, "[INFO] Distinct matched values: %s\n", fmt_num(*tally_distinct).c_str());
    fprintf(stderr, "[INFO] Throughput: %.2f MB/s\n", secs > 0 ? (double)t.bytes / 1e6 / secs : 0.0);
    fprintf(stderr, "[INFO] Total time: %.2fs\n", secs);
    fprintf(stderr, "[INFO] Query rate: %.0f queries/s\n", secs > 0 ? (double)t.candidates / secs : 0.0);
    std::string dl;
    for (int d : devs) { if (!dl.empty()) dl += ","; dl += std::to_string(d); }
    fprintf(stderr, "\n[INFO] === Devices ===\n[INFO] HIP devices: %s (%zu scanner%s, batches of %zu MiB)\n", dl.c_str(), devs.size(),
            devs.size() == 1 ? "" : "s", o.batch_bytes >> 20);
    if (o.render_gpu) fprintf(stderr, "[INFO] Rendered %zu batches on the GPU (%llu bytes of NDJSON), %zu fell back to the host renderer\n", pl.gpu_batches.load(), pl.gpu_bytes.load(), pl.gpu_fallback.load());
    if (o.pack) fprintf(stderr, "[INFO] Packed %zu inputs into %zu batches (%llu bytes of input in all)\n", packed.inputs, packed.packs, t.bytes);
    if (o.gz_gpu) fprintf(stderr, "[INFO] Inflated %zu .gz inputs on the GPU in %zu batches (%llu -> %llu bytes), %zu read on the host\n", gzr.on_gpu, gzr.packs,
                          gzr.packed_bytes, gzr.text_bytes, gzr.on_host);
    if (o.gz_members) fprintf(stderr, "[INFO] gz members on the GPU: %zu in %zu multi-member files\n", gzr.multi_members, gzr.multi_files);
    if (o.gz_stream_windows) fprintf(stderr, "[INFO] gz stream windows on the GPU: %zu windows of %zu files, %zu finished on the host\n", gzr.sw_windows, gzr.sw_files, gzr.sw_host);
    if (o.gz_windows) fprintf(stderr, "[INFO] gz windows on the GPU: %zu windows of %zu files, %zu finished on the host\n", gzr.win_windows, gzr.win_files, gzr.win_host);
    if (pl.u16_inputs.load())
        fprintf(stderr, "[INFO] UTF-16: %zu inputs transcoded on the GPU in %zu batches (%llu code units, %llu U+FFFD written; count %.2f ms, prefix %.2f ms, write %.2f ms)\n",
                pl.u16_inputs.load(), pl.u16_batches.load(), pl.u16_units.load(), pl.u16_replaced.load(), pl.u16_ms[0], pl.u16_ms[1], pl.u16_ms[2]);
    if (o.unescape_modes)
        fprintf(stderr, "[INFO] Unescape: %zu batches decoded on the GPU (%llu -> %llu bytes; %llu escapes, %llu U+FFFD written, %llu LF escapes as spaces; count %.2f ms, prefix %.2f ms, write %.2f ms)\n",
                pl.ue_batches.load(), pl.ue_in_bytes.load(), pl.ue_text_bytes.load(), pl.ue_counters[0].load(), pl.ue_counters[1].load(), pl.ue_counters[2].load(), pl.ue_ms[0],
                pl.ue_ms[1], pl.ue_ms[2]);
}

}  // namespace

int cmd_match(int argc, char** argv) {
    MatchOptions o;
    const int status = parse_match_options(argc, argv, o);
    if (status >= 0) return status;
    std::vector<int> devs;
    if (!expand_devices(o, devs)) return 1;
    const auto t0 = std::chrono::steady_clock::now();
    matchy_t* db = open_database(o.pos[0]);
    if (!db) return 1;
    const bool trace = getenv("MATCHY_AMD_TRACE") != nullptr;
    auto since0 = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    if (trace) fprintf(stderr, "[matchy] database open after %.1f ms\n", since0());
    uint32_t mask = 0;
    if (!o.extractors.empty()) {
        uint32_t auto_mask = 0;
        if (matchy_has_ip_data(db)) auto_mask |= MATCHY_EXTRACT_IPV4 | MATCHY_EXTRACT_IPV6;
        if (matchy_has_literal_data(db) || matchy_has_glob_data(db))
            auto_mask |= MATCHY_EXTRACT_DOMAINS | MATCHY_EXTRACT_EMAILS | MATCHY_EXTRACT_HASHES | MATCHY_EXTRACT_BITCOIN | MATCHY_EXTRACT_ETHEREUM | MATCHY_EXTRACT_MONERO;
        std::string err;
        if (!parse_extractors(o.extractors, auto_mask, mask, err)) { fprintf(stderr, "Error: %s\n", err.c_str()); matchy_close(db); return 1; }
    }
    // The pipeline: one worker and scanner per device entry inside the library (the first scanner is created here and now, so a device
    // that cannot be used fails the command; the others when the first batch reaches their workers — a small input never pays for
    // scanners it does not use)
    std::vector<int32_t> dev32(devs.begin(), devs.end());
    matchy_multi_scanner_t* ms = matchy_multi_scanner_create(db, mask, dev32.data(), dev32.size());
    if (!ms) {
        fprintf(stderr, "Error: Failed to create the GPU scanner on device %d: %s\n", devs[0], matchy_amd_last_error());
        matchy_close(db);
        return 1;
    }
    if (trace) fprintf(stderr, "[matchy] first of %zu scanner(s) created after %.1f ms\n", devs.size(), since0());
    MatchPipeline pl;
    pl.ms = ms;
    pl.json = o.format == "json";
    // --gz-on-gpu without records to render: no text comes back from a gz pack, so "Lines with matches" is counted on the GPU for every
    // batch (line context; with --format summary it changes nothing that is printed)
    // (--encoding and --unescape likewise: the text of such a batch is made on the device and stays there when nothing is rendered from it)
    pl.line_ctx = o.line_numbers || o.input_line || ((o.gz_gpu || o.encoding_given || o.unescape_modes) && !pl.json);
    pl.unescape_modes = o.unescape_modes;
    pl.input_line = o.input_line; pl.gather = o.gather_lines; pl.gz_members = o.gz_members; pl.whole_lines = o.whole_lines;
    pl.render_gpu = o.render_gpu;   // takes effect with --format json only (MatchPipeline::arm)
    if (pl.line_ctx) matchy_multi_scanner_set_line_context(ms, true);
    if (pl.gather) matchy_multi_scanner_set_hit_lines(ms, true);
    if (o.tally) matchy_multi_scanner_set_tally(ms, true);
    if (o.whole_lines) matchy_multi_scanner_set_whole_lines(ms, true);
    if (o.gz_pieces) (void)matchy_multi_scanner_set_gz_pieces(ms, o.gz_pieces);   // tested by parse_match_options
    matchy_multi_scanner_set_batch_hook(ms, &MatchPipeline::batch_hook, &pl);
    std::vector<std::string> paths;
    bool stdin_seen = false;
    for (size_t i = 1; i < o.pos.size(); ++i) {
        if (o.pos[i] == "-") {
            if (stdin_seen) { if (o.stats) fprintf(stderr, "[WARN] Skipping duplicate stdin argument\n"); continue; }
            stdin_seen = true;
        }
        paths.push_back(o.pos[i]);
        pl.sources.push_back(o.pos[i] == "-" ? "stdin" : o.pos[i]);
    }
    Totals t;
    std::vector<char> input_failed(paths.size(), 0);
    pl.line_base.assign(paths.size(), 0);
    pl.consumed.assign(paths.size(), -1);
    HostReader host{pl, paths, o.batch_bytes, std::vector<char>(paths.size(), 0), o.encoding};
    GzReader gzr(pl, host, o.gz_members, o.gz_windows, o.gz_pieces, o.gz_stream_windows);
    PackStats packed;
    run_inputs(o, pl, host, gzr, packed, t, input_failed);
    uint64_t tally_distinct = 0;
    const bool tally_failed = o.tally && !report_tally(ms, db, o.tally_limit, tally_distinct);
    fflush(stdout);
    if (trace) fprintf(stderr, "[matchy] all batches done after %.1f ms\n", since0());
    pl.release_mappings((size_t)-1);
    if (o.follow) {
        matchy_scanner_t* fsc = matchy_scanner_create(db, mask, devs[0]);
        if (!fsc) fprintf(stderr, "Error: Failed to create the GPU scanner on device %d: %s\n", devs[0], matchy_amd_last_error());
        else { matchy_scanner_set_line_context(fsc, pl.line_ctx); matchy_scanner_set_hit_lines(fsc, pl.gather); matchy_scanner_set_whole_lines(fsc, o.whole_lines); follow_inputs(pl, fsc, paths, o.stats, t); matchy_scanner_free(fsc); }
    }
    size_t failed = 0;
    for (char f : input_failed) failed += f != 0;
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (o.stats) report_stats(o, pl, gzr, packed, t, devs, paths.size() - failed, failed, secs, o.tally && !tally_failed ? &tally_distinct : nullptr);
    matchy_multi_scanner_free(ms);
    matchy_close(db);
    if (trace) fprintf(stderr, "[matchy] cleaned up after %.1f ms\n", since0());
    if (failed) { fprintf(stderr, "Error: %zu file(s) failed to process\n", failed); return 1; }
    return tally_failed ? 1 : 0;
}
