// Percent- and JSON-escaped inputs (unescape.hip): launch wrappers of the decoding kernels and the pass class a scanner owns. The rules
// are unescape_core.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hip_owners.h"
#include "line_index.h"
#include "unescape_core.h"

namespace mxy {

// Tiles one workgroup of the prefix step covers: the prefix kernels are those of the line index (tile_prefix_build).
constexpr uint32_t UNESCAPE_SCAN_CHUNK = LINE_SCAN_CHUNK;
// Tiles one workgroup of the state scan covers (JSON: esc at every tile's first byte)
constexpr uint32_t UNESCAPE_STATE_CHUNK = 2048;
static_assert(unescape::TILE_BYTES == LINE_TILE, "the tile geometry of line_index.hip: one 16-byte load of every lane of a wave");

// What the device knows about a decoded batch, in a 128-byte line of its own; the first 16 bytes come back to the host.
struct alignas(128) UnescapeCounters { uint32_t text_len, escapes, replaced, lf_escapes; };

uint32_t unescape_state_chunks(uint32_t n_tiles);
// JSON only. state[t] = the 7-bit state of tile t (unescape_core.h), t < tiles(len). codes: tiles(len) entries, fns: unescape_state_chunks(..).
hipError_t unescape_states(const uint8_t* data, uint32_t len, uint32_t* codes, uint32_t* fns, uint8_t* state, hipStream_t stream);
// counts[t] = output bytes of tile t; the counters grow by the escapes of the input. `data` is 16-byte aligned; mode: one of MODE_*;
// state: what unescape_states wrote (JSON), not read otherwise.
hipError_t unescape_count(const uint8_t* data, uint32_t len, uint32_t mode, const uint8_t* state, uint32_t* counts, UnescapeCounters* ctr, int n_cu, hipStream_t stream);
// ctr->text_len = prefix[n_tiles]
hipError_t unescape_seal(const uint32_t* prefix, uint32_t n_tiles, UnescapeCounters* ctr, hipStream_t stream);
// text[prefix[t] .. prefix[t + 1]) = the bytes of tile t; `text` is 16-byte aligned and holds prefix[n_tiles] bytes
hipError_t unescape_write(const uint8_t* data, uint32_t len, uint32_t mode, const uint8_t* state, const uint32_t* prefix, uint8_t* text, int n_cu, hipStream_t stream);

// The decoding pass of a scanner (Scanner::unescape): owns its buffers, grown on demand and reused between batches. Not thread-safe, like
// the scanner. Throws mxy::HipError, and mxy::ParamError for an input it refuses.
class Unescape {
public:
    // Throws ParamError for an input the pass refuses (modes, no input, the 2^31 bound): the test every entry makes first.
    static void check(const uint8_t* src, size_t len, uint32_t modes);
    // Room for an input that has to be copied to the device first (host memory, or device memory that is not 16-byte aligned).
    uint8_t* input_buffer(size_t len);
    // Queues the steps on `stream` and returns when the text's length is known on the host: the 16-byte counter block is copied to pinned
    // memory behind the prefix step, the write step is queued, and the host waits for the copy alone. modes = JSON | PERCENT: the JSON
    // run's text is the PERCENT run's input (the two text buffers take turns), and the host waits once per run. `src`: device memory,
    // 16-byte aligned (the caller's, or input_buffer() filled on `stream`).
    void launch(const uint8_t* src, size_t len, uint32_t modes, int n_cu, bool profile, hipStream_t stream);
    const uint8_t* device_text() const { return text_[cur_].p; }
    uint32_t text_len() const { return text_len_; }
    // with_text: the decoded batch is copied once to pinned host memory
    void queue_results(bool with_text, hipStream_t stream);
    // Behind the wait for `stream`. `text` is BORROWED from the pinned block (null without with_text) until the next launch().
    struct Result { const uint8_t* text = nullptr; size_t text_len = 0; uint64_t escapes = 0, replaced = 0, lf_escapes = 0; };
    Result finish();
    // milliseconds of count (JSON: with the state steps in front of it), prefix and write of the last profiled launch(), summed over its runs
    void timing(float out_ms[3]) const { for (int k = 0; k < 3; ++k) out_ms[k] = ms_[k]; }

private:
    void run(const uint8_t* in, uint32_t len, uint32_t mode, uint8_t* text, int n_cu, Event* ev, hipStream_t stream);
    DevBuf<uint8_t> in_, text_[2], state_;      // the input where it has to be copied; the texts: the input's length + 16 spare bytes
    DevBuf<uint32_t> counts_, chunks_, prefix_, codes_, fns_;
    DevBuf<UnescapeCounters> ctr_;
    PinnedBuf<UnescapeCounters> host_;
    PinnedBuf<uint8_t> text_pinned_;
    Event ev_len_;                              // behind the copy of the counter block
    Event ev_[2][4];                            // created by the first profiled launch(); one row per run
    float ms_[3] = {0, 0, 0};
    uint32_t text_len_ = 0, cur_ = 0, runs_ = 0;
    bool timed_ = false, with_text_ = false;
};

}  // namespace mxy
