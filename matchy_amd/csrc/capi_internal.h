// What capi.cpp and multi_scanner.cpp share behind the C ABI, and nothing else.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/matchy_amd.h"
#include "tally.h"

namespace mxy {
namespace capi {

void set_error(const std::string& e);           // the calling thread's matchy_amd_last_error()
int default_device_of(const matchy_t* db);      // the HIP device a handle's scanners use when none is named
// why matchy_scanner_scan_gz_window / matchy_multi_scanner_submit_gz_window refuse these arguments; nullptr: they do not
const char* gz_window_refusal(const uint8_t* packed, size_t packed_len, const matchy_gz_window_t* window);
// the same for matchy_scanner_scan_gz_stream / matchy_multi_scanner_submit_gz_stream (pieces off is the scanner's to refuse)
const char* gz_stream_refusal(const uint8_t* packed, size_t packed_len, const matchy_gz_stream_window_t* window);

// the 2^31 bound of matchy_scanner_scan_utf16 / matchy_multi_scanner_submit_utf16 and their byte_order test
const char* utf16_refusal(const uint8_t* data, size_t len, uint32_t byte_order);
// the same for matchy_scanner_scan_escaped / matchy_multi_scanner_submit_escaped: modes, no input, the length bound
const char* unescape_refusal(const uint8_t* data, size_t len, uint32_t modes);

struct ScanResultInternal {
    std::vector<matchy_scan_hit_t> hits;
    std::vector<uint32_t> ids;
    std::vector<int64_t> offs;
    bool on_device = false;   // MATCHY_SCAN_FETCH_DEVICE: the result's arrays are device pointers
    // line context (matchy_scan_result_lines): `lines` / `ip4_lines` point at the owned vector, at the scanner's pinned block
    // (borrowed results) or into device memory (on_device), like the hit arrays of the same result
    bool has_lines = false;
    std::vector<matchy_scan_line_t> lines_own;
    const matchy_scan_line_t* lines = nullptr;
    const matchy_scan_line_t* ip4_lines = nullptr;
    uint64_t lines_with_matches = 0;
    // segmented scan (matchy_scan_result_segments): the table is always owned; the per-record indices follow the hit arrays of the
    // same result like the line arrays do
    bool has_segments = false;
    std::vector<matchy_scan_segment_t> segments;
    std::vector<uint32_t> segment_of_own;
    const uint32_t* segment_of_hit = nullptr;
    const uint32_t* segment_of_ip4_hit = nullptr;
    // hit lines (matchy_scan_result_hit_lines): the block and its arrays point into the owned vectors, at the scanner's pinned blocks
    // (borrowed results) or into device memory (on_device), like the hit arrays of the same result; all NULL for a counts-only fetch
    bool has_hit_lines = false;
    matchy_scan_hit_lines_t hit_lines{};
    std::vector<uint8_t> hl_text_own;
    std::vector<uint32_t> hl_index_own;   // line_off, line_no, line_of_hit end to end
    // rendered records (matchy_scan_result_ndjson): the block follows the hit arrays of the same result — the scanner's pinned block, an
    // owned copy (render_own), or device memory (on_device)
    bool has_render = false;
    std::vector<uint8_t> render_own;
    const uint8_t* render_text = nullptr;
    uint64_t render_len = 0;
    int32_t render_status = 0;
    // gz scan (matchy_scan_result_gz): the statuses are always owned; the text is the scanner's pinned block, or owned (gz_text_own)
    // where the hit arrays are
    bool has_gz = false;
    std::vector<int32_t> gz_status;
    std::vector<uint8_t> gz_text_own;
    const uint8_t* gz_text = nullptr;
    size_t gz_text_len = 0;
    // scan behind a front pass (matchy_scan_result_utf16, matchy_scan_result_unescaped): the text the pass wrote is the scanner's pinned
    // block, or owned (front_text_own) where the hit arrays are
    bool has_utf16 = false, has_unescaped = false;
    std::vector<uint8_t> front_text_own;
    const uint8_t* front_text = nullptr;
    size_t front_text_len = 0;
    uint64_t utf16_code_units = 0, utf16_replaced = 0;
    uint64_t unescape_counters[3] = {0, 0, 0};   // escapes, replaced, lf_escapes
    // gz scan of files (matchy_scan_result_gz_files): one verdict per file and the members of file f, [first_member[f], first_member[f + 1]); owned
    bool has_gz_files = false;
    std::vector<int32_t> gz_file_status;
    std::vector<uint32_t> gz_first_member;
    // gz scan of a window (matchy_scan_result_gz_window): MATCHY_WINDOW_* and the partial line behind the window's last '\n'; owned
    bool has_gz_window = false;
    int32_t gz_window_status = 0;
    std::vector<uint8_t> gz_carry;
    // gz scan of a stream window (matchy_scan_result_gz_stream): the verdict and, for an OK window, the state behind it; the carry is
    // gz_carry; owned
    bool has_gz_stream = false, gz_stream_ended = false;
    int32_t gz_stream_status = 0, gz_stream_gz_status = 0;
    uint64_t gz_stream_consumed_bits = 0;
    uint32_t gz_stream_text_len = 0;
    std::vector<matchy_gz_stream_state_t> gz_stream_state;   // one, or none
    // gz scan with pieces on (matchy_scan_result_gz_pieces): the piece table and the pieces of member i, [first[i], first[i + 1]); owned
    bool has_gz_pieces = false;
    std::vector<matchy_gz_piece_t> gz_pieces;
    std::vector<uint32_t> gz_first_piece;
};

// hit tally (tally.h) behind matchy_scanner_tally_top / matchy_multi_scanner_tally_top
// the first `limit` entries of a scanner's tally (0 = all) and its totals; false when the scanner never enabled it. Throws what the engine throws.
bool scanner_tally_top(matchy_scanner_t* s, size_t limit, std::vector<TallyEntry>& rows, uint64_t& distinct, uint64_t& matches);
// hands `rows` (in their final order) to the caller as a matchy_tally_t that owns them
void fill_tally(std::vector<TallyEntry>&& rows, uint64_t distinct, uint64_t matches, matchy_tally_t* out);

}  // namespace capi
}  // namespace mxy
