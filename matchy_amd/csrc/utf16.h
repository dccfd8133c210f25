// UTF-16 inputs (utf16.hip): launch wrappers of the transcoding kernels and the pass class a scanner owns. The rules are utf16_core.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hip_owners.h"
#include "line_index.h"
#include "utf16_core.h"

namespace mxy {

// Tiles one workgroup of the prefix step covers: the prefix kernels are those of the line index (tile_prefix_build).
constexpr uint32_t UTF16_SCAN_CHUNK = LINE_SCAN_CHUNK;
static_assert(utf16::TILE_BYTES == LINE_TILE, "the tile geometry of line_index.hip: one 16-byte load of every lane of a wave");

// What the device knows about a transcoded batch, in a 128-byte line of its own; the first 16 bytes come back to the host.
struct alignas(128) Utf16Counters { uint32_t text_len, code_units, replaced, reserved; };

// counts[t] = output bytes of tile t (utf16::tiles(len) entries); ctr->replaced grows by the U+FFFD of the input. `data` is 16-byte aligned.
hipError_t utf16_count(const uint8_t* data, uint32_t len, uint32_t order, uint32_t* counts, Utf16Counters* ctr, int n_cu, hipStream_t stream);
// ctr->text_len = prefix[n_tiles], ctr->code_units = len / 2
hipError_t utf16_seal(const uint32_t* prefix, uint32_t n_tiles, uint32_t len, Utf16Counters* ctr, hipStream_t stream);
// text[prefix[t] .. prefix[t + 1]) = the bytes of tile t; `text` is 16-byte aligned and holds prefix[n_tiles] bytes
hipError_t utf16_write(const uint8_t* data, uint32_t len, uint32_t order, const uint32_t* prefix, uint8_t* text, int n_cu, hipStream_t stream);

// The transcoding pass of a scanner (Scanner::utf16_transcode): owns its buffers, grown on demand and reused between batches. Not
// thread-safe, like the scanner. Throws mxy::HipError, and mxy::ParamError for an input it refuses.
class Utf16Transcode {
public:
    // Throws ParamError for an input the pass refuses (byte order, no input, the 2^31 bound): the test every entry makes first.
    static void check(const uint8_t* src, size_t len, uint32_t order);
    // Room for an input that has to be copied to the device first (host memory, or device memory that is not 16-byte aligned).
    uint8_t* input_buffer(size_t len);
    // Queues count, prefix and write on `stream` and returns when the text's length is known on the host: the 16-byte counter block is
    // copied to pinned memory behind the prefix step, the write step is queued, and the host waits for the copy alone. `src`: device
    // memory, 16-byte aligned (the caller's, or input_buffer() filled on `stream`).
    void launch(const uint8_t* src, size_t len, uint32_t order, int n_cu, bool profile, hipStream_t stream);
    const uint8_t* device_text() const { return text_.p; }
    uint32_t text_len() const { return text_len_; }
    // with_text: the UTF-8 batch is copied once to pinned host memory
    void queue_results(bool with_text, hipStream_t stream);
    // Behind the wait for `stream`. `text` is BORROWED from the pinned block (null without with_text) until the next launch().
    struct Result { const uint8_t* text = nullptr; size_t text_len = 0; uint64_t code_units = 0, replaced = 0; };
    Result finish();
    // milliseconds of count, prefix and write of the last profiled launch()
    void timing(float out_ms[3]) const { for (int k = 0; k < 3; ++k) out_ms[k] = ms_[k]; }

private:
    DevBuf<uint8_t> in_, text_;                 // the input where it has to be copied; the text: the bound of the input + 16 spare bytes
    DevBuf<uint32_t> counts_, chunks_, prefix_;
    DevBuf<Utf16Counters> ctr_;
    PinnedBuf<Utf16Counters> host_;
    PinnedBuf<uint8_t> text_pinned_;
    Event ev_len_;                              // behind the copy of the counter block
    Event ev_[4];                               // created by the first profiled launch()
    float ms_[3] = {0, 0, 0};
    uint32_t text_len_ = 0;
    bool timed_ = false, with_text_ = false;
};

}  // namespace mxy
