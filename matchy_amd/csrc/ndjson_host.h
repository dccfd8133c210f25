// The host renderer of scan results: the records of a result as NDJSON, one line per record in the order of the arrays (hits, then
// compact IPv4 records) — the default output of `matchy match` (match_processor/parallel.rs:297-369). The record grammar is
// render::record_emit (render_core.h); this unit is one of its users, with a sink that appends to a std::string. It knows the plain
// record structs of the C ABI and nothing of HIP, the engine or the database image: payload JSON comes from a callback.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <unordered_map>

#include "../../include/matchy_amd.h"

namespace mxy {
namespace ndjson {

// payload JSON of a data offset ("null" where the value does not decode): NdjsonRender::PayloadFn
struct Payloads { void (*fn)(const void* ctx, uint32_t data_off, std::string& json); const void* ctx; };

// A host-resident result, as plain arrays. An array the result does not have is NULL, and its count is then not read.
struct ResultView {
    const matchy_scan_hit_t* hits = nullptr;
    const matchy_scan_ip4_hit_t* ip4_hits = nullptr;
    size_t n_hits = 0, n_ip4_hits = 0;
    const int64_t* data_offsets = nullptr;
    const matchy_scan_line_t *lines = nullptr, *ip4_lines = nullptr;              // line context, one per record
    const uint32_t *segment_of_hit = nullptr, *segment_of_ip4_hit = nullptr;      // segmented scans, one per record
    const matchy_scan_segment_t* segments = nullptr;
    size_t n_segments = 0;
    const matchy_scan_hit_lines_t* block = nullptr;   // hit lines: the records' text is read from the block (needs the line arrays)
    const uint8_t* text = nullptr;                    // the batch; may be NULL where the block serves
};

// What goes into a record beside the hit. with_lines: the line number (and with_input_line the input line) of the record, which
// record_emit puts between the payload and the match type (keys stay sorted). sources != NULL: the source of a record is
// sources[its segment], and its line number counts inside its segment: line_bases[s] + (line - segments[s].line_base) + 1.
// Otherwise `source` (NULL: "-") and line_base + line + 1.
struct Keys {
    const char* source = nullptr;
    const char* const* sources = nullptr;
    bool with_lines = false, with_input_line = false;
    uint64_t line_base = 0;
    const uint64_t* line_bases = nullptr;
};

// One per scanner: the rendered data payloads are cached by data offset (indicator lists carry a few hundred distinct payloads for
// millions of hits: decoding the MMDB value and serialising it per hit was most of the rendering time) and the last source is kept
// escaped, so a line costs a few appends. Use it from one thread at a time.
class Renderer {
public:
    // Every record of `v` in ONE malloc block (*out, NUL behind *out_len bytes; the caller frees it). Returns a MATCHY_* status; on
    // failure `error` says why.
    int32_t render(const ResultView& v, const Keys& k, Payloads pay, char** out, size_t* out_len, std::string& error);
    // Record i of `hits` (in_hits) or of `ip4_hits`: its line of render() without line keys and without the '\n'. Reads the block
    // where that has the record's line and the batch otherwise; false when neither is there. Touches no cache.
    static bool record(const ResultView& v, bool in_hits, size_t i, const char* source, Payloads pay, std::string& out);
    bool cached(uint32_t data_off) const { return json_of_data_.count(data_off) != 0; }

private:
    std::unordered_map<uint32_t, std::string> json_of_data_;   // at most 2^20 entries, then it starts over
    std::string source_, source_of_;                           // the last source, JSON-escaped, and its name
};

}  // namespace ndjson
}  // namespace mxy
