// Host driver of a chain of stream windows (inflate_core.h "windows of one stream", inflate_pieces.hip): one DEFLATE stream that is
// larger than a batch is handed to the device window by window. This header decides where the next window starts, how many compressed
// bytes it gets and when the chain is over; the device decides where a window ends (the open chain). Host only and header-only, like
// gz_packer.h: the command line, the Python mirror (matchy_amd.GzStreamWalker follows it line by line) and the CPU driver of the tests
// share this one rule.
//
// A window starts at byte `at` of the file with its first block at bit `bit` of that byte; the first window starts at byte 0, the gzip
// header included (the pass parses it), with flag FIRST. It gets a fixed guess of compressed bytes at first (first_bytes); behind an accepted window the
// walker follows the ratio that window showed: the bytes that would fill text_cap, an eighth more and a piece, since the device cuts at
// text_cap anyway — a wrong guess costs time and never correctness. No window is shorter than GZ_STREAM_MIN_PIECES pieces or longer than
// window_bytes (the caller's buffers are sized by it). A window that would leave less than a quarter of itself behind takes the rest of
// the file and carries FILE_END: only such a window may see the stream end. The chain is over behind a window that ended the stream and
// behind the first window that is not OK; what is left from (at, bit) on is then the caller's to finish.
#pragma once

#include <algorithm>
#include <cstdint>

namespace mxy {

constexpr uint32_t GZ_STREAM_FIRST = 1, GZ_STREAM_FILE_END = 2;   // MATCHY_STREAM_FIRST, MATCHY_STREAM_FILE_END
constexpr uint32_t GZ_STREAM_MIN_PIECES = 4;

struct GzStreamWindow { uint64_t offset, len; uint32_t bit, flags; };

struct GzStreamWalker {
    uint64_t file_len = 0;
    uint32_t window_bytes = 0, piece_bytes = 0, text_cap = 0;
    uint64_t at = 0, text_bytes = 0, want = 0;   // want: compressed bytes of the next window
    uint32_t bit = 0, windows = 0;
    bool over = false, ended = false;

    GzStreamWalker() = default;
    // first_bytes: the fixed guess for the first window (0: window_bytes, the bound of every window)
    GzStreamWalker(uint64_t file_len_, uint32_t window_bytes_, uint32_t piece_bytes_, uint32_t text_cap_, uint32_t first_bytes = 0)
        : file_len(file_len_), window_bytes(window_bytes_), piece_bytes(piece_bytes_), text_cap(text_cap_), want(first_bytes ? first_bytes : window_bytes_) { over = file_len == 0; }

    uint64_t clamp(uint64_t bytes) const {
        const uint64_t lo = std::min<uint64_t>((uint64_t)GZ_STREAM_MIN_PIECES * piece_bytes, window_bytes);
        return std::max(lo, std::min<uint64_t>(bytes, window_bytes));
    }
    // the window to send next (not over)
    GzStreamWindow next() const {
        const uint64_t left = file_len - at, w = clamp(want);
        GzStreamWindow out{at, w, bit, windows == 0 ? GZ_STREAM_FIRST : 0u};
        if (left <= w + w / 4) { out.len = left; out.flags |= GZ_STREAM_FILE_END; }
        return out;
    }
    // behind a window that came back OK: consumed_bits counts from bit 0 of the window's first byte. False (and the chain is over):
    // the device claims to have consumed nothing, or more than the window held.
    bool accept(const GzStreamWindow& w, uint64_t consumed_bits, uint32_t text_len, bool stream_ended) {
        ++windows;
        if (consumed_bits <= w.bit || consumed_bits > w.len * 8u) { over = true; return false; }
        const uint64_t bytes = consumed_bits / 8u;
        at = w.offset + bytes; bit = (uint32_t)(consumed_bits % 8u);
        text_bytes += text_len;
        // bytes / text_len compressed bytes per byte of text: what fills text_cap, an eighth more, and a piece
        const uint64_t fill = text_len ? (std::max<uint64_t>(bytes, 1) * text_cap + text_len - 1) / text_len : window_bytes;
        want = clamp(fill + fill / 8 + piece_bytes);
        if (stream_ended) { over = true; ended = true; }
        return true;
    }
    // behind a window that is not OK: the chain stops in front of it
    void refuse() { ++windows; over = true; }
};

}  // namespace mxy
