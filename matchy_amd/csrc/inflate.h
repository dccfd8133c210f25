// gz scans (inflate.hip): a pack of whole gzip files crosses the bus compressed, one wave per file inflates it into its segment of one
// batch in device memory, and the scan that exists runs over that batch. Launch wrappers, what host and kernels share, and the pass.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "gz_plan.h"
#include "hip_owners.h"
#include "inflate_core.h"

namespace mxy {

// One member as the kernels see it (GzPlanned without the host's status): body / body_len in the compressed buffer, start / cap in the batch.
// reserved[0]: the member's file in a scan of multi-member files (gz_plan_files), 0 otherwise. reserved[1], reserved[2]: the first piece
// and the piece count of a member that is split (inflate_pieces.hip), 0 and 0 otherwise.
struct GzMemberDev { uint64_t body; uint32_t body_len, start, cap, reserved[3]; };
static_assert(sizeof(GzMemberDev) == 32, "one member per 32-byte sector");

// Waves (64-thread workgroups) of k_gz_inflate that are resident on one CU at a time.
int gz_inflate_waves_per_cu();
// One wave per member of order[0, n_order), claimed from *counter (zeroed by the caller, on a 128-byte line of its own): inflates
// packed[body, body + body_len) to text[start, start + cap), verifies CRC-32 and ISIZE and writes the member's status. status[] holds
// the host's verdict on entry; members outside `order` keep it. Nothing is loaded outside packed[0, packed_len) or stored outside
// text[0, text_len).
hipError_t gz_inflate_launch(const uint8_t* packed, uint64_t packed_len, const GzMemberDev* members, uint32_t n_members, const uint32_t* order, uint32_t n_order,
                             uint32_t* counter, uint8_t* text, uint32_t text_len, int32_t* status, int grid, hipStream_t stream);
// One wave per member: the separator '\n' behind an OK member, the whole region of a failed one (separator included) set to '\n'.
hipError_t gz_seal_launch(const GzMemberDev* members, uint32_t n_members, const int32_t* status, uint8_t* text, uint32_t text_len, hipStream_t stream);
// Multi-member files, behind k_gz_inflate in place of the seal. The members of file f are [first_member[f], first_member[f + 1]) and
// carry f in reserved[0].
// One wave per file: file_status[f] = OK if all its members are OK, otherwise the status of its first member in stream order that is not.
hipError_t gz_file_verdict_launch(const uint32_t* first_member, uint32_t n_files, const int32_t* status, uint32_t n_members, int32_t* file_status, hipStream_t stream);
// One wave per member, behind the verdict on the same stream: the region of a member of a failed file is set to '\n'; the last member of
// a file whose capacity is not 0 writes the separator '\n' behind the file, in both outcomes.
hipError_t gz_seal_files_launch(const GzMemberDev* members, uint32_t n_members, const uint32_t* first_member, uint32_t n_files, const int32_t* file_status,
                                uint8_t* text, uint32_t text_len, hipStream_t stream);

// Windows (gz_plan_window): behind k_gz_seal_files on the same stream, one workgroup of GZ_TAIL_THREADS for the one window of the batch,
// whose text is text[0, seg_end) with carry_len bytes of carry in front. It finds the window's last '\n' within the last carry_cap + 1
// bytes, walking back in blocks of GZ_TAIL_BLOCK bytes, copies the partial line behind it (the tail, at most carry_cap bytes) to
// carry_out and overwrites it with '\n'; result[0] = the tail's length, result[1] = GZ_WINDOW_OK or GZ_WINDOW_NO_LINE_END (the whole
// window is then '\n'). A window whose file_status[0] is not OK gets its carry region set to '\n' as well, and `last` (the file ends
// here) cuts nothing and writes the separator at text[seg_end]. Nothing is loaded or stored outside text[0, text_len) and
// carry_out[0, carry_cap).
constexpr uint32_t GZ_TAIL_THREADS = 256, GZ_TAIL_BLOCK = 4096;
constexpr int32_t GZ_WINDOW_OK = 0, GZ_WINDOW_NO_LINE_END = 1;
hipError_t gz_window_tail_launch(uint8_t* text, uint32_t text_len, uint32_t seg_end, uint32_t carry_len, const int32_t* file_status, uint32_t carry_cap, bool last,
                                 uint8_t* carry_out, uint32_t* result, hipStream_t stream);

// Pieces of one stream (inflate_pieces.hip, gz_plan_pieces): what the seven kernels share. pieces / starts have n_pieces entries, laid out
// member by member (GzMemberDev::reserved[1..2]); split[0, n_split) are the split members; complete / failed / crc have one word per
// member; scratch[0, scratch_len) are the 16-bit symbols, a member's at gz::Piece::sym_base. The launches run in this order on one
// stream, behind the copies of packed bytes and tables: find, count, chain, symbols, windows, resolve, verdict. The verdict writes
// GZ_OK for a member whose pieces gave its text, and for every other split member its index into handover[0, n_split) — filled up with
// 0xFFFFFFFF — which gz_inflate_launch then takes as its order list. Nothing is loaded outside packed[0, packed_len), nothing stored
// outside text[0, text_len), scratch[0, scratch_len) and the tables.
struct GzPieceArgs {
    const uint8_t* packed; uint64_t packed_len;
    const GzMemberDev* members; uint32_t n_members;
    gz::Piece* pieces; uint64_t* starts; uint32_t n_pieces, piece_bytes;
    const uint32_t* split; uint32_t n_split;
    uint32_t *complete, *failed, *crc;
    uint16_t* scratch; uint64_t scratch_len;
    uint8_t* text; uint32_t text_len;
};
hipError_t gz_piece_find_launch(const GzPieceArgs& a, hipStream_t stream);
hipError_t gz_piece_count_launch(const GzPieceArgs& a, hipStream_t stream);
hipError_t gz_piece_chain_launch(const GzPieceArgs& a, hipStream_t stream);
hipError_t gz_piece_symbols_launch(const GzPieceArgs& a, hipStream_t stream);
hipError_t gz_piece_windows_launch(const GzPieceArgs& a, hipStream_t stream);
hipError_t gz_piece_resolve_launch(const GzPieceArgs& a, hipStream_t stream);
hipError_t gz_piece_verdict_launch(const GzPieceArgs& a, int32_t* status, uint32_t* handover, hipStream_t stream);

// Windows of one stream (inflate_pieces.hip "stream windows"; the rules: inflate_core.h "windows of one stream"). One window is
// in[0, in_len), compressed bytes of one DEFLATE stream whose first block starts at bit `bit` of in[0]; *state is the text in front of
// it (all zero for the first window; bit and history_len are also passed by value, tested by the host). The batch is
// batch[0, batch_len) = [carry_len bytes of carry][text_cap bytes for the window's text]['\n'], the scratch has text_cap symbols.
// The launches run in this order on one stream behind the copies of the compressed bytes, the state and the carry and a zeroed *dev:
// find, count, chain, symbols, windows, resolve, verdict, tail. The verdict writes dev->status / gz_status, on STREAM_OK *state_out and
// '\n' over everything behind the text, otherwise '\n' over the whole batch; the tail (k_gz_window_tail's rule, with the text's end
// and "the stream ended here" read from *dev) then hands the partial line behind the last '\n' out. Nothing is loaded outside
// in[0, in_len), nothing stored outside batch[0, batch_len), scratch[0, text_cap), the tables, *dev and *state_out.
struct GzStreamDev {
    uint64_t consumed_bits;              // the chain: the end bit of the last live piece, relative to in[0]
    uint32_t n_live, text_len, ended;
    int32_t chain_failed;                // gz::StreamChain::failed
    uint32_t bad, crc;                   // a marker pointed in front of the history; xor of the pieces' CRC parts (both zeroed by the host)
    int32_t status, gz_status;           // the verdict: gz::STREAM_*, and the MATCHY_GZ_* value of STREAM_FAILED
    uint32_t reserved[2];                // 48 bytes: the host zeroes whole 16-byte units
};
static_assert(sizeof(GzStreamDev) == 48, "three 16-byte units");
struct GzStreamArgs {
    const uint8_t* in; uint32_t in_len, bit, history_len;
    gz::Piece* pieces; uint64_t* starts; uint32_t n_pieces, piece_bytes;
    const gz::StreamState* state; gz::StreamState* state_out; GzStreamDev* dev;
    uint16_t* scratch;
    uint8_t* batch; uint32_t batch_len, carry_len, text_cap, file_end;
};
hipError_t gz_stream_find_launch(const GzStreamArgs& a, hipStream_t stream);
hipError_t gz_stream_count_launch(const GzStreamArgs& a, hipStream_t stream);
hipError_t gz_stream_chain_launch(const GzStreamArgs& a, hipStream_t stream);
hipError_t gz_stream_symbols_launch(const GzStreamArgs& a, hipStream_t stream);
hipError_t gz_stream_windows_launch(const GzStreamArgs& a, hipStream_t stream);
hipError_t gz_stream_resolve_launch(const GzStreamArgs& a, hipStream_t stream);
hipError_t gz_stream_verdict_launch(const GzStreamArgs& a, hipStream_t stream);
// result[0] = the tail's length, result[1] = GZ_WINDOW_OK or GZ_WINDOW_NO_LINE_END, as for gz_window_tail_launch
hipError_t gz_stream_tail_launch(uint8_t* batch, uint32_t batch_len, uint32_t carry_len, uint32_t text_cap, const GzStreamDev* dev, uint32_t carry_cap, uint8_t* carry_out,
                                 uint32_t* result, hipStream_t stream);
constexpr int GZ_STREAM_PASSES = 8;   // find, count, chain, symbols, windows, resolve, verdict, tail

// The gz pass of a scanner (Scanner::gz_inflate): the plan of the pack in flight and the buffers of the pass, grown on demand and reused
// between scans. A scan runs as launch() in front of the scan's kernels, queue_results() behind them on the same stream and finish()
// behind the wait. Not thread-safe, like the scanner. Throws mxy::HipError and, for a table that breaks its rules, mxy::ParamError.
class GzInflate {
public:
    // Plans the pack (gz_plan.h), queues the copies of the compressed bytes and the tables, k_gz_inflate and k_gz_seal on `stream`.
    void launch(const uint8_t* packed, size_t packed_len, const GzMemberIn* members, size_t n, int n_cu, bool profile, hipStream_t stream);
    // The same for a pack of files of one member or many (gz_plan_files): k_gz_inflate over the members of all files, then
    // k_gz_file_verdict and k_gz_seal_files. starts() are then the FILES' starts: file i is segment i.
    void launch_files(const uint8_t* packed, size_t packed_len, const GzFileIn* files, size_t n_files, int n_cu, bool profile, hipStream_t stream);
    // One window of a file that is larger than a batch: packed[0, packed_len) are its whole members (gz_plan_window), carry[0, carry_len)
    // the partial line the window in front left behind, staged through a pinned block of the pass and copied to text[0, carry_len).
    // k_gz_inflate over the members, k_gz_file_verdict and k_gz_seal_files for the one file, then k_gz_window_tail. The window is
    // segment 0 of the scan.
    void launch_window(const uint8_t* packed, size_t packed_len, const uint8_t* carry, uint32_t carry_len, uint32_t carry_cap, bool last, int n_cu, bool profile,
                       hipStream_t stream);
    // One window of one DEFLATE stream that is larger than a batch (GzStreamArgs above). packed[0, packed_len) are the window's compressed
    // bytes; with `first` they begin with the gzip header, which is parsed here (a header that does not parse: STREAM_FAILED with
    // GZ_BAD_HEADER, nothing is launched but the fill), and state is not read; otherwise *state is the state the window in front handed
    // out. The batch is [carry][text_cap bytes][one '\n'], segment 0 of the scan. Pieces must be on. On the device: the eight passes,
    // no host round trip between them.
    void launch_stream(const uint8_t* packed, size_t packed_len, const gz::StreamState* state, const uint8_t* carry, uint32_t carry_len, uint32_t carry_cap, uint32_t text_cap,
                       bool first, bool file_end, int n_cu, bool profile, hipStream_t stream);
    // Pieces of one stream: 0 = off (the default), otherwise a power of two in [GZ_PIECE_BYTES_MIN, GZ_PIECE_BYTES_MAX]
    // (gz_piece_bytes_valid). From the next launch on, every member of at least 2 * piece_bytes compressed bytes is split
    // (gz_plan_pieces) and inflated by one wave per piece; with 0 no piece kernel is launched and nothing of them is allocated.
    void set_pieces(uint32_t piece_bytes) { piece_bytes_ = piece_bytes; }
    uint32_t pieces() const { return piece_bytes_; }
    const uint8_t* device_text() const { return text_.p; }
    uint32_t text_len() const { return (uint32_t)plan_.total; }
    const std::vector<uint32_t>& starts() const { return plan_.starts; }
    // The statuses, and with want_text the inflated batch, come back into pinned memory.
    void queue_results(bool want_text, hipStream_t stream);
    // Behind the wait for `stream`. status / text are BORROWED from the pinned blocks and valid until the next launch(); text is null
    // without want_text (text_len is the length of the batch either way). ok_bytes: inflated bytes of the OK members; not_input_nl: the '\n' bytes of the batch that are not the input's
    // (separators and the regions of failed members).
    // Behind launch_files() the accounting is per file (a file is OK when all its members are), and file_status (n_files values),
    // first_member (n_files + 1) are set: borrowed like status.
    struct Result { const int32_t* status = nullptr; size_t n = 0; const uint8_t* text = nullptr; size_t text_len = 0; uint64_t ok_bytes = 0, not_input_nl = 0;
                    const int32_t* file_status = nullptr; size_t n_files = 0; const uint32_t* first_member = nullptr;
                    // behind launch_window(): the window's status (GZ_WINDOW_*) and its carry, borrowed like status. ok_bytes is then
                    // carry_len + capacities - carry_len of the result (0 for a failed window or NO_LINE_END), not_input_nl the rest of the batch
                    bool window = false; int32_t window_status = 0; const uint8_t* carry = nullptr; uint32_t carry_len = 0;
                    // pieces of one stream: the table of the launch (empty with pieces off or no member split), borrowed like status;
                    // the pieces of member i are [first_piece[i], first_piece[i + 1]), n + 1 entries
                    const gz::Piece* pieces = nullptr; size_t n_pieces = 0; const uint32_t* first_piece = nullptr;
                    // behind launch_stream(): the window's status (gz::STREAM_*; STREAM_NO_LINE_END is the tail's), the MATCHY_GZ_* value of
                    // a failed one, the bits consumed from packed[0] on (header included), the window's text length, whether the stream ended
                    // in it, and the state behind it (borrowed like status; meaningful for STREAM_OK only). status[0] is stream_gz_status,
                    // carry / carry_len, ok_bytes and not_input_nl are as behind launch_window()
                    bool stream = false; int32_t stream_status = 0, stream_gz_status = 0; uint64_t consumed_bits = 0; uint32_t stream_text_len = 0; bool ended = false;
                    const gz::StreamState* state_out = nullptr; };
    Result finish();
    // milliseconds of k_gz_inflate (CRC included: it runs in the same kernel), 0, and k_gz_seal (k_gz_file_verdict + k_gz_seal_files
    // behind launch_files) of the last profiled launch
    void timing(float out_ms[3]) const { for (int k = 0; k < 3; ++k) out_ms[k] = ms_[k]; }
    // behind launch_window() the third value includes k_gz_window_tail; this is that kernel's own time (0 behind any other launch)
    float tail_ms() const { return tail_ms_; }
    // pieces: find, count, chain, symbols, windows + resolve + verdict, handover inflate of the last profiled launch; zeros with pieces
    // off or no member split. (These times are part of timing()'s first value.)
    void pieces_timing(float out_ms[6]) const { for (int k = 0; k < 6; ++k) out_ms[k] = piece_ms_[k]; }
    // stream windows: find, count, chain, symbols, windows, resolve, verdict, tail of the last profiled launch_stream(); zeros otherwise
    void stream_timing(float out_ms[GZ_STREAM_PASSES]) const { for (int k = 0; k < GZ_STREAM_PASSES; ++k) out_ms[k] = stream_ms_[k]; }

private:
    void inflate_files(GzFilesPlan& fp, const uint8_t* packed, size_t packed_len, int n_cu, bool profile, hipStream_t stream);
    void upload_and_inflate(const uint8_t* packed, size_t packed_len, int n_cu, bool profile, hipStream_t stream);
    GzPlan plan_;                 // behind launch_files: members and order of all files, starts of the files
    bool files_ = false;          // the launch in flight was launch_files
    std::vector<uint32_t> first_member_host_, file_caps_;
    DevBuf<uint32_t> first_member_;
    DevBuf<int32_t> file_status_;
    PinnedBuf<int32_t> file_status_pinned_;
    std::vector<GzMemberDev> members_host_;
    std::vector<int32_t> status_host_;
    DevBuf<uint8_t> packed_, text_;
    DevBuf<GzMemberDev> members_;
    DevBuf<uint32_t> order_, counter_;
    DevBuf<int32_t> status_;
    PinnedBuf<int32_t> status_pinned_;
    PinnedBuf<uint8_t> text_pinned_;
    Event ev_[3];                 // created by the first profiled launch()
    // windows: set by launch_window, never allocated without it
    bool window_ = false, window_last_ = false;
    uint32_t carry_len_ = 0, carry_cap_ = 0;
    DevBuf<uint8_t> carry_out_;
    DevBuf<uint32_t> window_result_;
    PinnedBuf<uint8_t> carry_in_pinned_, carry_out_pinned_;
    PinnedBuf<uint32_t> window_result_pinned_;
    Event ev_tail_;
    float tail_ms_ = 0;
    // pieces of one stream: nothing below is allocated while piece_bytes_ is 0
    void inflate_pieces(size_t packed_len, int n_cu, bool profile, hipStream_t stream);
    uint32_t piece_bytes_ = 0;
    GzPiecePlan piece_plan_;
    std::vector<gz::Piece> pieces_host_;
    DevBuf<gz::Piece> pieces_;
    DevBuf<uint64_t> piece_starts_;
    DevBuf<uint32_t> split_, handover_, member_words_, handover_counter_;   // member_words_: complete, failed, crc
    DevBuf<uint16_t> scratch_;
    PinnedBuf<gz::Piece> pieces_pinned_;
    Event ev_piece_[7];
    bool pieces_timed_ = false;
    float piece_ms_[6] = {0, 0, 0, 0, 0, 0};
    // stream windows: nothing below is allocated without launch_stream
    void queue_stream_results(bool want_text, hipStream_t stream);
    Result finish_stream();
    bool stream_ = false, stream_timed_ = false;
    uint64_t stream_body_ = 0;
    int32_t stream_host_status_ = 0, stream_host_gz_ = 0;   // decided in front of the kernels (the header, no bytes behind it): then nothing is launched
    uint32_t stream_text_cap_ = 0;
    DevBuf<gz::StreamState> stream_state_;     // [0] the state handed in, [1] the state handed out
    DevBuf<GzStreamDev> stream_dev_;
    PinnedBuf<gz::StreamState> stream_state_pinned_;   // [0] staging of the state handed in, [1] the state handed out
    PinnedBuf<GzStreamDev> stream_dev_pinned_;
    Event ev_stream_[GZ_STREAM_PASSES + 1];
    float stream_ms_[GZ_STREAM_PASSES] = {0, 0, 0, 0, 0, 0, 0, 0};
    float ms_[3] = {0, 0, 0};
    bool timed_ = false, with_text_ = false;
    int waves_per_cu_ = 0;
};

}  // namespace mxy
