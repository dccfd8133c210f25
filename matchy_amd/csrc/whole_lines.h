// Whole-line queries (whole_lines.hip): the front end that turns the LINES of a batch into candidates on the device, in place of
// k_anchor and the validators — launch wrappers and the constants the host sizes its buffers with. The rules are in whole_lines_core.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "line_index.h"
#include "scan_types.h"

namespace mxy {

// The units of the streaming pass: a wave takes one tile per step, 16 bytes per lane (the tiles of line_index.hip, whose '\n' prefix
// the pass reads), and a workgroup a chunk of consecutive tiles per round.
constexpr uint32_t WL_TILE = 1024;
constexpr uint32_t WL_LANE_BYTES = 16;
constexpr uint32_t WL_WG_CHUNK = 16384;
static_assert(WL_TILE == LINE_TILE && WL_TILE == 64 * WL_LANE_BYTES && WL_WG_CHUNK % (4 * WL_TILE) == 0, "whole tiles per wave of a 256-thread workgroup");

// Counters of the mode for one scan, in device memory (zeroed in front of the pass). Address queries (low half) and string queries
// (high half) share one 64-bit word: a workgroup of the classify kernel reports both with ONE atomic — atomics on one line are served
// one after the other, and with four per wave of 8192 waves scatter + classify took 0.48 ms for 10 M lines where they now take 0.42.
struct WholeLineCounters {
    unsigned long long address_string;
    uint32_t queries, invalid_utf8;
    uint32_t address() const { return (uint32_t)address_string; }
    uint32_t string() const { return (uint32_t)(address_string >> 32); }
};

struct WholeLineParams {
    const uint8_t* data;
    uint32_t len;
    const uint32_t* prefix;   // exclusive '\n' prefix over the tiles (line_index_build), line_tiles(len) + 1 entries
    uint32_t* ends;           // position of the r-th '\n', `cap` entries
    uint8_t* invalid;         // 1: line r holds a byte that is not valid UTF-8, `cap` entries (zeroed in front of the pass)
    Candidate* cands;         // candidate r is query r, `cap` entries
    uint32_t cap;
    WholeLineCounters* wl;
    ScanCounters* counters;   // n_cand = the lines of the batch (may exceed cap: nothing is written behind it), lines, error
    PackParams pk;            // IPv6 queries are looked up by the classify kernel itself and leave through pack_record
};

// k_wl_scatter: second streaming pass. Every '\n' at position p with rank r writes ends[r] = p; every byte that is not valid UTF-8
// marks the line it lies in. Nothing is written at or behind `cap`.
void launch_whole_lines_scatter(const WholeLineParams& p, int n_cu, hipStream_t stream);
// k_wl_classify: one lane per line. Strips the '\r', classifies the query and writes its candidate: IPv4 with the address, strings as
// IT_DOMAIN with pad 0, a list sentinel for what the lookup passes must not touch (invalid UTF-8, IPv6 — answered here).
void launch_whole_lines_classify(const WholeLineParams& p, const DevDb& db, int n_cu, hipStream_t stream);

}  // namespace mxy
