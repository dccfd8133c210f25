// Host pipeline around the HIP kernels: PSL table, device-resident database image, scan sessions.
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "db_image.h"
#include "extract_render.h"
#include "hip_owners.h"
#include "hit_lines.h"
#include "inflate.h"
#include "line_index.h"
#include "render.h"
#include "result_layout.h"
#include "scan_types.h"
#include "segments.h"
#include "unescape.h"
#include "utf16.h"
#include "whole_lines.h"

namespace mxy {

// kernel launch wrappers (k_anchor.hip, validate_kernels.hip, lookup_kernels.hip)
int anchor_blocks_per_cu();
int validate_blocks_per_cu(bool ac);
void launch_anchor(const TokParams& p, const DevDb& db, int grid, hipStream_t stream);
void launch_validate_dom(const TokParams& p, const DevDb& db, int grid, hipStream_t stream);
void launch_validate_misc(const TokParams& p, const DevDb& db, int grid, hipStream_t stream);
void launch_rare(const TokParams& p, const DevDb& db, int grid, hipStream_t stream);
void launch_lookup(const LookupParams& p, const DevDb& db, int grid, hipStream_t stream);
void launch_lookup_early_glob(const LookupParams& p, const DevDb& db, int grid, hipStream_t stream);
void launch_lookup_ip(const LookupParams& p, const DevDb& db, int grid, bool dense, hipStream_t stream);
// k_lookup_spill over p.spill (launched by Scanner::fetch when a scan has spilled candidates); threads = spill_threads() per block
void launch_lookup_spill(const LookupParams& p, const DevDb& db, hipStream_t stream);
uint32_t spill_threads();
// ip_tables.hip: the /24 table + /24 bitmap, and the leaf tables of the undecided /24s, built on the device from the uploaded tree
void launch_ip_l24(const uint2* nodes, uint32_t node_count, uint32_t v4_start, uint2* l24, uint32_t* bm24, uint32_t* n_undecided, hipStream_t s);
void launch_ip_leaf(const uint2* nodes, uint32_t node_count, uint2* l24, uint32_t* next, uint32_t n_leaf, uint32_t* leaf_node, uint2* leaf, hipStream_t s);

class DistinctSet;   // distinct.h
class HitTally;      // tally.h
struct TallyEntry;

// Public-suffix set loaded from the PSLB container (tools/gen_psl.py), shared by all handles.
struct PslHost {
    std::vector<std::string> suffixes;
    std::vector<PslSlot> slots;
    std::vector<uint8_t> pool;
    std::vector<uint32_t> bloom;
    std::vector<uint2> tld_tab;   // exact table of the last labels of <= 7 bytes (see DevDb::tld_tab)
    std::vector<uint2> tld_pfx;   // exact table of the first 8 bytes of the last labels of >= 8 bytes (see DevDb::tld_pfx)
    uint32_t mask = 0, max_tld_len = 0, max_suffix_len = 0;
    uint32_t tld_first[8] = {0};
    static const PslHost& get();  // throws std::runtime_error if the container cannot be found
};

// Device-resident image of one database on one GPU (uploaded once, at first use).
struct DeviceDb {
    int device = 0;
    DevDb view{};
    DevBuf<uint2> ip_nodes, ip_l1, ip_l24, ip_leaf;
    DevBuf<uint32_t> ip_bm24, lit_bm, sfx_bm;
    DevBuf<uint2> tld_tab, tld_pfx;
    DevBuf<uint32_t> dfa, dfa_node;
    DevBuf<uint8_t> dfa_cls;
    DevBuf<LitSlot> lit_slots;
    DevBuf<uint8_t> lit_pool, pg, psl_pool;
    DevBuf<uint32_t> lit2pat_off, lit2pat, bloom;
    DevBuf<uint32_t> lit_offsets, glob_offsets;  // pattern id -> data-section offset (pack_record)
    DevBuf<PslSlot> psl_slots;
    DevBuf<uint32_t> lc_map;
    DevBuf<uint2> lc_ign, lc_cased;
    uint32_t n_lit_offsets = 0, n_glob_offsets = 0;
    size_t bytes_uploaded = 0;
    void upload(const DbImage& img, int dev);
};

// HIP-event intervals of the last scan. One stream: k_anchor | k_validate_dom + k_validate | k_rare | lookups incl. record packing.
// Forked scan (three streams): anchor_ms as before, validate_ms = everything behind k_anchor, rare_ms = lookup_ms = 0.
// Sliced scan: anchor_ms = first k_anchor launch to the end of the last (the other slices' tails run beside), validate_ms = what is
// left behind the last k_anchor.
struct ScanTiming { float anchor_ms = 0, validate_ms = 0, rare_ms = 0, lookup_ms = 0, total_ms = 0; int slices = 1; };

enum HitMode { HITS_NONE = 0, HITS_FINAL = 1, HITS_RAW = 2 };

struct ScanOutput {
    std::vector<Candidate> cands;  // filled only when requested
    std::vector<Hit> hits;         // HITS_RAW (single-query path)
    std::vector<uint32_t> ids;
    // HITS_FINAL: dense records produced by pack_record, BORROWED from the scanner's pinned buffers
    // (valid until the next scan on that scanner)
    const FinalHit* fin = nullptr;
    const uint32_t* fin_ids = nullptr;
    const long long* fin_offs = nullptr;
    size_t n_fin = 0, n_fin_ids = 0;
    // compact IPv4 records of a scan with `compact` set (they are NOT in fin then), BORROWED like fin
    const uint2* c4 = nullptr;
    size_t n_c4 = 0;
    uint64_t lines = 0;
    uint32_t n_cand = 0, n_hits = 0;
    uint64_t by_type[IT_COUNT] = {0};
    // line context (ScanRequest::lines): one record per entry of fin / c4, BORROWED like them (HITS_FINAL; otherwise the arrays stay
    // on the device: Scanner::device_lines), and the number of distinct lines that carry a hit
    bool has_lines = false;
    const LineRec* fin_lines = nullptr;
    const LineRec* c4_lines = nullptr;
    uint64_t lines_with_matches = 0;
    // segmented scan (Scanner::set_segments): the table, and one segment index per entry of fin / c4. A scan_device fetch BORROWS them
    // like fin (the indices stay on the device unless HITS_FINAL: Scanner::device_segment_of); scan_host owns them in seg_own / seg_of_own,
    // with indices and line_base in the caller's table and buffer
    bool has_segments = false;
    const SegmentRec* segments = nullptr;
    size_t n_segments = 0;
    const uint32_t* seg_of_fin = nullptr;
    const uint32_t* seg_of_c4 = nullptr;
    std::vector<SegmentRec> seg_own;
    std::vector<uint32_t> seg_of_own;
    // hit lines (ScanRequest::hit_lines): the block of the distinct lines with a hit and its index arrays (hit_lines.h). A scan_device
    // fetch BORROWS them like fin (device pointers unless HITS_FINAL); scan_host owns them in hl_*_own, merged over its pieces
    bool has_hit_lines = false;
    HitLinesView hit_lines;
    std::vector<uint8_t> hl_text_own;
    std::vector<uint32_t> hl_off_own, hl_no_own, hl_of_own;
    // rendered records (ScanRequest::render): the NDJSON block of the records of this fetch, BORROWED like fin (a device pointer unless
    // HITS_FINAL); scan_host owns it in render_own, the blocks of its pieces end to end
    RenderView render;
    std::vector<uint8_t> render_own;
    // candidates as text (Scanner::set_extract_text): the output of `matchy extract` for the candidates of this fetch, in pinned host memory,
    // BORROWED like fin; scan_host hands out the blocks of its pieces end to end, with the counts summed. `cands` stays empty then.
    ExtractTextView extract_text;
};

// Process-wide registry of the host ranges this library pinned (hipHostRegister): the caller's (matchy_amd_host_register, kept until
// matchy_amd_host_unregister) and the transient ones Scanner::scan_host pins around its copies. Reference-counted, so that a range two
// scanners copy from at the same time is unpinned when the LAST copy is done — never under a DMA another thread has in flight — and a
// range is only ever treated as pinned when an entry of the registry covers ALL of it. Memory pinned by someone else (hipHostMalloc,
// a foreign hipHostRegister) is not in the registry: scan_host copies from it with one plain hipMemcpyAsync and leaves the choice of
// path to the runtime, which knows.
namespace pins {
// returns true when [a, b) is pinned for the caller until release(a, b): covered by an entry (its count goes up) or registered now.
bool acquire(uintptr_t a, uintptr_t b);
void release(uintptr_t a, uintptr_t b);
// caller-owned entries (matchy_amd_host_register / _unregister); 0 = success
int add_caller(const void* ptr, size_t bytes);
void remove_caller(const void* ptr);
}

// Merge the dense records of a piece that starts `base` bytes into the whole: starts move by `base`, a glob record (kind 3: `value`
// is the index of its id list) moves behind the ids gathered so far. Hit is FinalHit or matchy_scan_hit_t (same layout, capi.cpp).
template <class Hit, class Off, class OffOut>
void append_shifted(const Hit* hits, size_t n_hits, const uint32_t* ids, const Off* offs, size_t n_ids, uint32_t base,
                    std::vector<Hit>& all_hits, std::vector<uint32_t>& all_ids, std::vector<OffOut>& all_offs) {
    const uint32_t id_shift = (uint32_t)all_ids.size();
    for (size_t i = 0; i < n_hits; ++i) {
        Hit h = hits[i];
        h.start += base;   // the whole is below 4 GiB (checked by the callers)
        if (h.kind == 3) h.value += id_shift;
        all_hits.push_back(h);
    }
    all_ids.insert(all_ids.end(), ids, ids + n_ids);
    all_offs.insert(all_offs.end(), offs, offs + n_ids);
}

// What Scanner::scan_device scans and how. `ptr` is `len` bytes resident in device memory (16-byte aligned), len < 2^31.
struct ScanRequest {
    const uint8_t* ptr = nullptr;
    uint32_t len = 0;
    bool lookup = false;       // false stops after extraction
    // pack_record also writes the final records into pinned host memory (unsorted fetches then need no copy)
    bool host_mirror = false;
    // run the parts of the scan that do not depend on each other on the scanner's extra streams (engine.cpp). For ONE batch at a
    // time on device-resident input; callers that keep several batches in flight (submit / wait) or whose time is the host-to-device
    // copy (scan_host) stay on one stream per scanner: the runtime multiplexes streams onto a few hardware queues, and three
    // scanners with three streams each ran 25 % slower than with one each.
    bool fork = false;
    int slices = 0;            // with fork: cut the batch into that many slices (see Scanner::MAX_SLICES); 0 = the default (one slice)
    bool compact = false;      // IPv4 results leave as 8-byte records (ScanOutput::c4, scan_types.h c4_pack) when compact_possible()
    bool lines = false;        // line context: fetch() resolves every final record to its line (line_index.hip); needs `lookup`
    bool hit_lines = false;    // fetch() packs the distinct lines with a hit into one block (hit_lines.hip); needs `lines`
    bool render = false;       // fetch() renders the records as NDJSON on the device (render.hip); set by Scanner::arm_render
    // every line of the batch is one query (whole_lines.hip) in place of extraction; needs `lookup`; set by Scanner::arm_whole_lines.
    // The scan runs on ONE stream: `fork` and `slices` are ignored in this mode.
    bool whole_lines = false;
};

// Moves the line records of a piece that starts `base` bytes and `line_base` lines into the whole (append_shifted for the line array).
template <class Line>
void append_shifted_lines(const Line* lines, size_t n, uint32_t base, uint32_t line_base, std::vector<Line>& all) {
    for (size_t i = 0; i < n; ++i) {
        Line l = lines[i];
        l.line += line_base; l.line_start += base; l.line_end += base;
        all.push_back(l);
    }
}

// Bytes of a piece of Scanner::scan_host: below 1 GiB, or what MATCHY_AMD_HOST_PIECE_BYTES says (read once, clamped to that maximum; tests
// of the piece arithmetic).
size_t host_piece_bytes();

// Payload JSON of the data record at `data_off` of the DbImage `img`, "null" where it does not decode: the one rule of both NDJSON renderers
// (NdjsonRender::PayloadFn, ndjson::PayloadFn).
void payload_json(const void* img, uint32_t data_off, std::string& json);

// A scan session: owns the per-launch work buffers on one device. Not thread-safe; create one per thread/stream.
class Scanner {
public:
    Scanner(std::shared_ptr<const DbImage> img, std::shared_ptr<DeviceDb> ddb, uint32_t extract_flags, uint32_t min_labels);
    ~Scanner();
    // Launches the scan of `rq` on `stream`. Results stay on the device until fetch().
    void scan_device(const ScanRequest& rq, hipStream_t stream);
    // the compact record holds data-section offsets of C4_DATA_BITS bits: every offset an IP result of this database can carry must fit
    bool compact_possible() const { return img_->max_ip_data_offset() < (1u << C4_DATA_BITS); }
    // Copies counters (and hits / candidates) back. Call after scan_device; synchronises the stream.
    // sorted: the final records are put into canonical order on the GPU (sort_hits.hip) before they are copied back
    void fetch(ScanOutput& out, bool want_cands, hipStream_t stream, HitMode hit_mode = HITS_FINAL, bool sorted = false);
    // One synthetic candidate (single-query API): `text` is uploaded, only the lookup kernel runs.
    // the dense hit records of the last lookup scan as the kernel left them in device memory (MATCHY_SCAN_FETCH_DEVICE)
    const FinalHit* device_final() const { return final_.p; }
    const uint32_t* device_final_ids() const { return final_ids_.p; }
    const long long* device_final_offs() const { return final_offs_.p; }
    size_t device_final_id_count() const { return host_counters_.n_final_ids; }
    // line context: scans launched through scan_host resolve lines when set (scan_device callers pass ScanRequest::lines)
    void set_line_context(bool on) { line_ctx_ = on; }
    bool line_context() const { return line_ctx_; }
    // the line records of the last scan with line context as the kernel left them in device memory, parallel to device_final() / the compact array
    const LineRec* device_lines() const { return lines_ ? lines_->device_lines() : nullptr; }
    const LineRec* device_c4_lines() const { return lines_ ? lines_->device_c4_lines() : nullptr; }
    // with set_profile: milliseconds of the streaming count kernel, of the prefix sum, and of resolve + distinct set of the last fetch
    void line_timing(float out_ms[3]) const { for (int k = 0; k < 3; ++k) out_ms[k] = 0; if (lines_) lines_->timing(out_ms); }
    // Hit lines (hit_lines.hip): scans launched through scan_host gather them when set, and resolve lines for it (scan_device callers
    // pass ScanRequest::hit_lines together with ::lines). Never set, nothing of it is allocated, launched or copied.
    void set_hit_lines(bool on) { hit_lines_on_ = on; }
    bool hit_lines() const { return hit_lines_on_; }
    // with set_profile: milliseconds of mark + rank + lengths + offsets, of the copy kernel, and of the block's device-to-host copy
    void hit_lines_timing(float out_ms[3]) const { for (int k = 0; k < 3; ++k) out_ms[k] = 0; if (hit_lines_) hit_lines_->timing(out_ms); }
    // Rendered records (render.hip): set_render arms the NEXT lookup scan (copied; null disarms). arm_render is what the entries of a
    // lookup scan call behind arm_segments and in front of scan_device: it consumes the pending parameters whether the scan succeeds or
    // not, checks them against the request (ParamError: line flags without line context, per-segment sources without segments or in
    // another number), queues the copy of the source table on `stream` and sets rq.render. fetch_renders false (a counts-only fetch):
    // nothing is rendered. Never armed, nothing of it is allocated, launched or copied.
    void set_render(const RenderParams* p);
    void arm_render(ScanRequest& rq, bool fetch_renders, hipStream_t stream);
    bool render_pending() const { return (bool)render_pending_; }
    // with set_profile: milliseconds of measure + offsets, of the write step, and of the block's device-to-host copy of the last fetch
    void render_timing(float out_ms[3]) const { for (int k = 0; k < 3; ++k) out_ms[k] = 0; if (render_) render_->timing(out_ms); }
    // repeats of the pass, payloads rendered and misses of the last fetch that rendered (null: none yet)
    const NdjsonRender::Events* render_events() const { return render_ ? &render_->last_events() : nullptr; }
    // Segmented scans (segments.hip): `starts` (copied) describes the buffer of the NEXT lookup scan as n segments — starts[0] == 0,
    // non-decreasing, every start <= the scan's length, every non-empty segment in front of the last ends in '\n'. n == 0 or null
    // clears a pending table. arm_segments(len) is what the entries of a lookup scan call before scan_device: it consumes the pending
    // table (none: the scan has no segments), checks it against `len`, throws ParamError for a bad one and queues its copy to the device
    // on `stream` in front of the scan. scan_host arms itself.
    // fetch() then attributes the records on the device and throws ParamError when a segment breaks the newline rule.
    void set_segments(const uint32_t* starts, size_t n);
    void arm_segments(size_t len, hipStream_t stream, bool upload = true);   // upload false: scan_host, which uploads piece by piece
    const uint32_t* device_segment_of() const { return segments_ ? segments_->device_of_fin() : nullptr; }
    const uint32_t* device_segment_of_c4() const { return segments_ ? segments_->device_of_c4() : nullptr; }
    // with set_profile: milliseconds of the segment pass, the record passes and the lines-with-matches pass of the last fetch
    void segment_timing(float out_ms[3]) const { for (int k = 0; k < 3; ++k) out_ms[k] = 0; if (segments_) segments_->timing(out_ms); }
    // gz scans (inflate.hip): gz_inflate plans the pack of whole gzip files (throws ParamError for a table that breaks its rules),
    // queues its copy, k_gz_inflate and k_gz_seal on this scanner's own stream and sets the segment table of the batch — member i is
    // segment i — for the lookup scan the caller then launches on that stream over (text, len). gz_queue_results goes behind the scan's
    // kernels, gz_finish behind the fetch. Never called, nothing of it is allocated, launched or copied.
    struct GzBatch { const uint8_t* text; uint32_t len; hipStream_t stream; };
    GzBatch gz_inflate(const uint8_t* packed, size_t packed_len, const GzMemberIn* members, size_t n);
    // the same for files of one member or many (GzInflate::launch_files): FILE i is segment i
    GzBatch gz_inflate_files(const uint8_t* packed, size_t packed_len, const GzFileIn* files, size_t n_files);
    // one window of a file that is larger than a batch (GzInflate::launch_window): the window is segment 0, its carry lies in front
    GzBatch gz_inflate_window(const uint8_t* packed, size_t packed_len, const uint8_t* carry, uint32_t carry_len, uint32_t carry_cap, bool last);
    // one window of one DEFLATE stream that is larger than a batch (GzInflate::launch_stream): the window is segment 0, its carry lies in
    // front; gz pieces must be on
    GzBatch gz_inflate_stream(const uint8_t* packed, size_t packed_len, const gz::StreamState* state, const uint8_t* carry, uint32_t carry_len, uint32_t carry_cap, uint32_t text_cap,
                              bool first, bool file_end);
    void gz_queue_results(bool want_text);
    GzInflate::Result gz_finish();
    // with set_profile: milliseconds of k_gz_inflate (CRC included), 0, and k_gz_seal of the last gz scan
    void gz_timing(float out_ms[3]) const { for (int k = 0; k < 3; ++k) out_ms[k] = 0; if (gz_) gz_->timing(out_ms); }
    // the same behind a window scan (the third value then includes k_gz_window_tail), and that kernel's own time as a fourth
    // pieces of one stream (inflate_pieces.hip): 0 = off, otherwise a valid piece size (gz_piece_bytes_valid; the C ABI tests it). It
    // holds for every gz_inflate* from the next one on: members of at least 2 * piece_bytes compressed bytes are inflated by many waves.
    void set_gz_pieces(uint32_t piece_bytes) { gz_piece_bytes_ = piece_bytes; }
    uint32_t gz_pieces() const { return gz_piece_bytes_; }
    void gz_pieces_timing(float out_ms[6]) const { for (int k = 0; k < 6; ++k) out_ms[k] = 0; if (gz_) gz_->pieces_timing(out_ms); }
    // stream windows: find, count, chain, symbols, windows, resolve, verdict, tail of the last profiled window
    void gz_stream_timing(float out_ms[GZ_STREAM_PASSES]) const { for (int k = 0; k < GZ_STREAM_PASSES; ++k) out_ms[k] = 0; if (gz_) gz_->stream_timing(out_ms); }
    void gz_window_timing(float out_ms[4]) const { gz_timing(out_ms); out_ms[3] = gz_ ? gz_->tail_ms() : 0; }
    // UTF-16 inputs (utf16.hip): utf16_transcode queues count, prefix and write on this scanner's own stream and returns, when the text's
    // length has reached the host, the UTF-8 batch in device memory for the lookup scan the caller then launches on that stream over
    // (text, len). `src` is host or device memory; byte_order: utf16::ORDER_LE / ORDER_BE. Segments and whole-line mode are not offered:
    // a pending segment table (dropped then) or whole-line mode fails the call with ParamError, as does an input whose bound reaches 2^31
    // bytes. utf16_queue_text goes behind the scan's kernels, utf16_finish behind the fetch. Never called, nothing of it is allocated,
    // launched or copied.
    GzBatch utf16_transcode(const uint8_t* src, size_t len, uint32_t byte_order);
    void utf16_queue_text(bool want_text);
    Utf16Transcode::Result utf16_finish();
    // milliseconds of count, prefix and write of the last transcoded batch (recorded for every batch, with or without set_profile)
    void utf16_timing(float out_ms[3]) const { for (int k = 0; k < 3; ++k) out_ms[k] = 0; if (utf16_) utf16_->timing(out_ms); }
    // Percent- and JSON-escaped inputs (unescape.hip): the contract of the three utf16_* members above. unescape queues the steps of the
    // pass on this scanner's own stream and returns, when the text's length has reached the host, the decoded batch in device memory;
    // modes: unescape::MODE_PERCENT, MODE_JSON or both (percent(json(x))). `src` is host or device memory. A pending segment table
    // (dropped then), whole-line mode, modes outside 1..3 and an input of 0x7FFF0000 bytes or more fail the call with ParamError.
    // unescape_queue_text goes behind the scan's kernels, unescape_finish behind the fetch. Never called, nothing of it is allocated,
    // launched or copied.
    GzBatch unescape(const uint8_t* src, size_t len, uint32_t modes);
    void unescape_queue_text(bool want_text);
    Unescape::Result unescape_finish();
    // milliseconds of count, prefix and write of the last decoded batch (recorded for every batch, with or without set_profile)
    void unescape_timing(float out_ms[3]) const { for (int k = 0; k < 3; ++k) out_ms[k] = 0; if (unescape_) unescape_->timing(out_ms); }
    // Whole-line queries (whole_lines.hip): while on, a lookup scan treats its buffer as a list of queries, one per line, and looks every
    // line up like Database::lookup does a single query; extraction (k_anchor, the validators, the extract flags) plays no part.
    // scan_host reads the setting itself; the other entries of a lookup scan call arm_whole_lines in front of arm_segments, which sets
    // rq.whole_lines and throws ParamError for a combination the mode does not have (segments, hit lines, rendered records; `gz`: the
    // caller is a gz scan) — pending segment tables and render parameters are dropped then. Never set, nothing of it is allocated,
    // launched or copied.
    void set_whole_lines(bool on) { whole_lines_ = on; }
    bool whole_lines() const { return whole_lines_; }
    void arm_whole_lines(ScanRequest& rq, bool gz = false);
    // queries, address queries, string queries and queries that are not valid UTF-8 of the last scan in the mode (scan_host: summed over its pieces)
    void whole_lines_counters(uint64_t out[4]) const { for (int k = 0; k < 4; ++k) out[k] = wl_ ? wl_->last[k] : 0; }
    // with set_profile: milliseconds of count + prefix, of scatter + classify, and of the lookups of the last scan in the mode
    void whole_lines_timing(float out_ms[3]) const { for (int k = 0; k < 3; ++k) out_ms[k] = wl_ ? wl_->ms[k] : 0; }
    // Distinct candidate texts (distinct.hip), for extractor handles: while on, a fetch with want_cands returns only the candidates whose
    // text this scanner has not returned since it was created or reset — the set lives in device memory across scans and pieces, and only
    // the survivors are copied back. Off (the default), nothing of it is allocated, launched or copied.
    void set_unique(bool on);
    bool unique() const { return unique_; }
    void reset_unique();
    uint64_t unique_count() const;
    // Candidates as text (extract_render.hip), for extractor handles: while a format is set (xrender::FORMAT_*; negative: off), a fetch of
    // an extraction scan with want_cands orders its candidates and writes the output of `matchy extract` on the device; ScanOutput::extract_text
    // is what comes back, and the candidate records stay where they are. With set_unique the block holds the first occurrences only. A
    // launch the order key does not hold is refused (XR_REFUSED) before the distinct set sees it. Off (the default), nothing of it is
    // allocated, launched or copied.
    void set_extract_text(int format) { extract_text_format_ = format; }
    int extract_text_format() const { return extract_text_format_; }
    // device milliseconds of keys + sort, measure, write and the block's copy of the last fetch that rendered candidates
    void extract_text_timing(float out_ms[4]) const { for (int k = 0; k < 4; ++k) out_ms[k] = 0; if (extract_render_) extract_render_->timing(out_ms); }
    uint64_t extract_text_allocations() const { return extract_render_ ? extract_render_->allocations() : 0; }
    // Hit tally (tally.hip): while on, every fetch of a lookup scan counts the final records of its batch per distinct (item type, matched
    // text) in a table that lives in device memory across scans and pieces; tally_top reads the first `limit` entries out (0 = all). Off
    // (the default), nothing of it is allocated, launched or copied; switching it off keeps what was counted.
    void set_tally(bool on);
    bool tally() const { return tally_on_; }
    void reset_tally();
    const HitTally* hit_tally() const { return tally_.get(); }   // null until the tally was first enabled
    void tally_top(size_t limit, std::vector<TallyEntry>& out);
    void lookup_one(const std::string& text, Candidate c, ScanOutput& out);
    // Convenience: host buffer -> internal device buffer -> scan -> fetch (chunks of < 2^31 bytes).
    // `fin*` vectors receive owned copies of the final hits of all pieces, positions made absolute.
    void scan_host(const uint8_t* data, size_t len, bool lookup, bool want_cands, ScanOutput& out, std::vector<uint64_t>* cand_bases,
                   std::vector<FinalHit>* fin, std::vector<uint32_t>* fin_ids, std::vector<long long>* fin_offs, std::vector<LineRec>* fin_lines = nullptr);
    void set_profile(bool on) { profile_ = on; }
    // slices of the forked scan_device: 0 = default for the batch size (one slice), 1 = never cut, n = n equal slices
    void set_slices(int n) { slices_ = n < 0 ? 0 : n; }
    int slices() const { return slices_; }
    int last_slice_count() const { return n_slices_; }
    const ScanTiming& timing() const { return timing_; }
    uint32_t flags() const { return flags_; }
    int device() const { return ddb_->device; }
    const DbImage& image() const { return *img_; }

    // A device-resident batch of one synchronous scan is cut into up to MAX_SLICES slices (byte ranges on SEG_ALIGN boundaries, no
    // newline alignment needed: positions stay absolute and k_anchor looks across the cuts): k_anchor runs slice after slice on the
    // scan's stream, and everything behind it (validation, lookups, result traffic) runs per slice on three side streams, i.e.
    // BESIDE k_anchor of the following slices. Every slice has its own work lists and counters; the final records of all slices
    // go to the same arrays (slots reserved with atomics on the counters of slice 0).
    static constexpr int MAX_SLICES = 8;
    static constexpr uint32_t SPILL_BLOCKS = 16;

private:
    // work lists of one slice (grown on demand, reused between scans)
    struct Work {
        DevBuf<Candidate> cands, cands_a;   // candidates of the validation kernels / IPv4 candidates of k_anchor
        DevBuf<Candidate> cands_m, cands_r, cands_d; // forked scans of databases without globs: candidates of the third stream (tokens, IPv6, e-mail) / of k_rare
        DevBuf<RareAnchor> rare, rare_dom, tok, heavy;
        DevBuf<uint32_t> dom_list;
        size_t dom_slots = 0;
        DevBuf<Hit> hits;                   // single-query path and the spill pass only
        DevBuf<uint32_t> ids, glob_work;
        DevBuf<uint32_t> glob_work_d;       // work list k_validate_dom fills itself (forked scans of glob databases)
        DevBuf<uint32_t> spill;             // glob candidates beyond the per-lane storage of the glob pass (k_lookup_spill)
        void ensure(uint32_t len);
    };
    Work work_[MAX_SLICES];
    int n_slices_ = 1;                      // slices of the last scan_device
    int slices_ = 0;                        // set_slices()
    void ensure_capacity(uint32_t len);     // slice 0 + the final arrays, for a scan of `len` bytes in one slice
    void ensure_final(size_t recs, size_t ids);
    // kernel parameters and grids of one slice of the last scan_device (kept: the spill pass is launched from fetch())
    struct SliceLaunch {
        TokParams tp;
        LookupParams lp, la, lm, lr, ld;   // lookups of the validation kernels' candidates / of k_anchor's IPv4 candidates / of the third stream's lists
        bool split_misc = false;   // the third stream has a candidate list and a lookup pass of its own
        int gm[3] = {1, 1, 1};
        int grid_anchor = 1, ip_grid = 1;
        bool ip_pass = false, ip_dense = false;
    };
    SliceLaunch launch_[MAX_SLICES];
    void slice_params(int sl, const ScanRequest& rq, uint32_t lo, uint32_t hi, SliceLaunch& L);
    int plan_slices(uint32_t len, int want, uint32_t (&cuts)[MAX_SLICES + 1]);
    void setup_spill(int sl, LookupParams& lp);
    // the launch schedules of scan_device: slices on the side streams / one slice forked onto them / everything on `stream`
    void launch_sliced(int ns, hipStream_t stream);
    void launch_forked(hipStream_t stream);
    void launch_one_stream(hipStream_t stream);
    void launch_whole_lines(const ScanRequest& rq, hipStream_t stream);   // the schedule of a scan in whole-line mode
    void ensure_dom_stream();       // the fourth stream and its events, created at first use
    bool rare_possible() const { return (flags_ & (EX_HASHES | EX_BITCOIN | EX_ETHEREUM | EX_MONERO)) != 0; }
    // the steps of fetch(), in its order
    void settle_counters(bool trace, hipStream_t stream);
    void report_counters(ScanOutput& out, bool trace);
    const FinalHit* queue_record_copies(ScanOutput& out, bool want_cands, HitMode hit_mode, bool sorted, hipStream_t stream);
    void queue_post_passes(ScanOutput& out, const FinalHit* dev_recs, bool want_cands, HitMode hit_mode, bool trace, hipStream_t stream);
    void finish_fetch(ScanOutput& out, bool want_cands, HitMode hit_mode, hipStream_t stream);
    // visits every (work list, counter) pair of a slice for fetch's overflow test and regrow
    template <class F> void each_list(Work& w, const ScanCounters& s, F&& f);
    bool spill_done_ = false;
    bool early_glob_ = false;       // last scan_device: the glob pass over k_validate_dom's flagged candidates runs beside the lean pass
    uint32_t expect_chains_ = 0;    // side-stream chains of the last scan_device that report their end to k_finish (0: event joins)
    // List sizes of the PREVIOUS scan of this scanner (fetch): the grids of the kernels behind the streaming pass are sized for the
    // sparse lists of a web-server log — half a workgroup per CU for the long tokens, an eighth for some lookups — and a log of another
    // shape (two file hashes per line: 18 M tokens) walked such a list with 500 iterations per lane. Batches of one input look alike,
    // so the next scan's grids follow the last scan's counts (grid_for); the first scan of a scanner runs with the defaults.
    struct ListHint { uint32_t n_tok = 0, n_rare = 0, n_rare_dom = 0, n_heavy = 0, n_cand = 0, n_cand_m = 0, n_cand_r = 0, n_cand_d = 0, n_dom = 0; } hint_;
    uint32_t dom_preset_ = 0;   // what ScanCounters::n_dom of slice 0 holds on the device while the counters are clean (k_finish presets it: TokParams::dom_static)
    uint32_t dom_want_ = 0;     // ... and what the scan in flight asked for
    int grid_for(uint32_t n_hint, uint32_t per_wg, int dflt, int max_per_cu) const;
    bool counters_clean_ = false;   // the device counter blocks are zero (k_finish of the last fetch left them so)
    ScanRequest last_;              // of the last scan_device (fetch runs it again after regrowing the work lists)
    std::shared_ptr<const DbImage> img_;
    std::shared_ptr<DeviceDb> ddb_;
    Stream host_stream_;            // scan_host: this scanner's own non-blocking stream, created by the first scan_host
    uint32_t flags_, min_labels_;
    // the lookups of k_anchor's IPv4 candidates run on this stream beside the validation kernels (fork after k_anchor, join
    // before the counters are read back)
    Stream aux_stream_;
    Event ev_fork_, ev_join_;
    // a third stream: k_validate's part that does not depend on k_validate_dom (tokens, IPv6 / e-mail anchors) and k_rare behind it
    Stream aux2_stream_;
    Event ev_join2_;
    // sliced scans: the k_validate_dom -> k_validate -> k_lookup chain of every slice runs on a stream of its own too (the scan's
    // stream only carries the k_anchor launches), one "k_anchor of slice i is done" and one "misc stream of slice i is done" event
    // per slice (all created at first use)
    Stream dom_stream_;
    Event ev_anchor_[MAX_SLICES], ev_misc_[MAX_SLICES];
    Event ev_join3_, ev_dom_, ev_v1_;
    DevBuf<FinalHit> final_;
    DevBuf<uint32_t> final_ids_;
    DevBuf<long long> final_offs_;
    DevBuf<unsigned long long> sort_keys_;
    DevBuf<uint32_t> sort_vals_;
    DevBuf<uint8_t> sort_tmp_;
    DevBuf<FinalHit> final_sorted_;
    DevBuf<ScanCounters> counters_;            // MAX_SLICES entries
    // the passes behind the scan, each created at first use: line context (line_index.h; line_ctx_ is what scan_host asks for),
    // hit lines (hit_lines.h),
    // segmented scans (segments.h), gz scans (inflate.h), distinct texts (distinct.h), hit tally (tally.h)
    bool line_ctx_ = false;
    std::unique_ptr<LineContext> lines_;       // created by the first fetch of a scan with line context
    bool hit_lines_on_ = false;
    std::unique_ptr<HitLines> hit_lines_;      // created by the first fetch of a scan with hit lines
    std::unique_ptr<SegmentPass> segments_;    // created by the first set_segments with a table
    std::unique_ptr<RenderParams> render_pending_;   // set_render, until arm_render takes it
    std::unique_ptr<NdjsonRender> render_;     // created by the first arm_render that arms a scan
    std::unique_ptr<GzInflate> gz_;            // created by the first gz_inflate
    uint32_t gz_piece_bytes_ = 0;
    std::unique_ptr<Utf16Transcode> utf16_;    // created by the first utf16_transcode
    // the pages of a host input that utf16_transcode pinned for its copy (pins::acquire), until utf16_finish or the next batch
    struct HostPin {
        uintptr_t a = 0, b = 0;
        void release();
        ~HostPin() { release(); }
    } utf16_pin_;
    std::unique_ptr<Unescape> unescape_;       // created by the first unescape
    HostPin unescape_pin_;                     // the same for unescape, until unescape_finish or the next batch
    // what utf16_transcode and unescape share: the input where the pass can read it (device memory, 16-byte aligned), queued on host_stream_
    template <class Pass> const uint8_t* front_pass_input(Pass& pass, HostPin& pin, const uint8_t* src, size_t len);   // engine.cpp only
    // what gz_inflate and gz_inflate_files share: device, stream, the pass; launch(GzInflate&) plans and queues; then the segment table
    template <class Launch> GzBatch gz_pass(Launch&& launch);   // engine.cpp only
    // whole-line queries: the buffers of the front end (grown with the candidate list, reused between scans), created by the first scan in the mode
    struct WholeLines {
        DevBuf<uint32_t> counts, chunks, prefix, ends;
        DevBuf<uint8_t> invalid;
        DevBuf<WholeLineCounters> ctr;
        PinnedBuf<WholeLineCounters> host;
        uint64_t last[4] = {0, 0, 0, 0};
        float ms[3] = {0, 0, 0};
    };
    bool whole_lines_ = false;
    std::unique_ptr<WholeLines> wl_;
    bool unique_ = false;
    std::unique_ptr<DistinctSet> distinct_;    // created by the first set_unique(true), kept (with its texts) while the feature is switched off
    int extract_text_format_ = -1;
    std::unique_ptr<ExtractRender> extract_render_;   // created by the first fetch that renders candidates
    bool tally_on_ = false;
    std::unique_ptr<HitTally> tally_;          // created by the first set_tally(true), kept (with its counts) while the feature is switched off
    DevBuf<uint32_t> spill_scratch_;           // per-thread scratch of k_lookup_spill (allocated when a scan first spills)
    DevBuf<uint8_t> staging_;  // scan_host only
    // pinned mirror of the final records written by the lookup kernels themselves, laid out by mirror_layout_ (result_layout.h)
    PinnedBuf<uint8_t> mirror_;
    ResultLayout mirror_layout_;
    bool mirror_used_ = false;
    void ensure_mirror(uint32_t recs, uint32_t ids);
    // compact IPv4 records (scan_device `compact`): device array, pinned mirror written by the kernels, pinned block of the copy path
    DevBuf<uint2> c4_;
    PinnedBuf<uint2> mirror_c4_, pinned_c4_;
    bool compact_ = false;   // of the last scan_device: in effect
    PinnedBuf<uint8_t> pinned_;   // one pinned block: a ResultLayout for the counts of the fetch (or Hit[n] for HITS_RAW)
    void ensure_pinned(size_t bytes) { pinned_.ensure(bytes, bytes / 4 + (1 << 16)); }
    ScanCounters host_counters_{};             // the slices' counters summed (list counters: of slice 0 for one-slice scans)
    PinnedBuf<ScanCounters> host_slices_;      // MAX_SLICES counter blocks as read back
    bool last_forked_ = false;
    bool single_ = false;
    bool profile_ = false;
    Event ev_[5];
    ScanTiming timing_;
    int n_cu_ = 256;
};

}  // namespace mxy
