// Line context of hit records (line_index.hip): launch wrappers and the constants the host sizes its buffers with.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mxy {

// Bytes per tile of the '\n' count array: one 16-byte load of every lane of a wave. The array costs 4 bytes per tile (0.4 % of the
// batch); a hit's walk over the bytes of its own tile in front of it costs half a tile on average, which is what a larger tile makes
// dearer.
constexpr uint32_t LINE_TILE = 1024;
// Tiles one workgroup of the prefix sum covers (2 MiB of log).
constexpr uint32_t LINE_SCAN_CHUNK = 2048;
constexpr uint32_t LINE_SET_EMPTY = 0xFFFFFFFFu;   // free slot of the distinct-line set (line numbers stay below 2^31)

// 0x80 in every byte of x that is '\n' (exact: no carry crosses a byte): the SWAR test of the '\n' counts, here and in segments.hip
#if defined(__HIPCC__)
__device__ __forceinline__ uint32_t nl_bytes(uint32_t x) {
    const uint32_t v = x ^ 0x0A0A0A0Au;
    return ~(((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v | 0x7F7F7F7Fu);
}
#endif

// One record per hit, bit-identical to matchy_scan_line_t (include/matchy_amd.h).
struct LineRec { uint32_t line, line_start, line_end, reserved; };

// The distinct-line counter of a scan in a 128-byte line of its own.
struct alignas(128) LineCounters { uint32_t distinct; };

uint32_t line_tiles(uint32_t len);
uint32_t line_chunks(uint32_t n_tiles);
// '\n' counts per tile and their exclusive prefix (counts: line_tiles(len) entries, chunk_sums: line_chunks(..), prefix: line_tiles(len) + 1).
// after_count: recorded behind the streaming count kernel when not null (timing).
hipError_t line_index_build(const uint8_t* data, uint32_t len, uint32_t* counts, uint32_t* chunk_sums, uint32_t* prefix, int n_cu, hipStream_t stream,
                            hipEvent_t after_count);
// out[i] for record i of `recs` (n records of `stride` = 16 or 8 bytes that begin with the start offset). set != nullptr: the line numbers
// also go into that set (set_slots: a power of two, at least twice the records of all calls that share it, filled with LINE_SET_EMPTY) and
// *n_distinct grows by the number of lines that were not in it yet.
hipError_t line_index_resolve(const uint8_t* data, uint32_t len, const uint32_t* prefix, const void* recs, uint32_t stride, uint32_t n, LineRec* out,
                              uint32_t* set, uint32_t set_slots, uint32_t* n_distinct, hipStream_t stream);

}  // namespace mxy
