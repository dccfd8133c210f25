// Device helpers shared by the validation and the lookup kernels: the IPv6 text parser and the flattened Aho-Corasick
// automaton (DbImage::build_ac_dfa) with its LDS-resident shallow part.
#pragma once
#include "device_common.h"

namespace mxy {

// SearchTree::lookup_v4 (matchy-format/src/mmdb/tree.rs:46-90). true + data offset + prefix length, or false for "not found".
// The first levels come from a table built at upload (DeviceDb::upload): the outcome of the first 24 levels for every /24 prefix
// (DevDb::ip_l24, 128 MB, when the tree is big enough to pay for it) and, for a /24 with entries below it, a leaf table with the
// outcome for each of its 256 addresses (ip_leaf) — two dependent loads per lookup. Small trees: the first 16 levels (ip_l1) and
// the reference's walk, one dependent 8-byte load per level.
struct IpTables { const uint2* l24; const uint2* l1; const uint2* leaf; const uint2* nodes; uint32_t node_count; };
__device__ __forceinline__ bool trie_v4_tables(const IpTables& t, uint32_t addr, uint32_t& data_off, uint32_t& prefix) {
    uint2 e = t.l24 ? t.l24[addr >> 8] : t.l1[addr >> 16];
    uint32_t kind = e.x & 0xFF;
    if (kind == 3) {   // leaf table of this /24: the outcome for each of its 256 addresses
        e = t.leaf[((size_t)e.y << 8) | (addr & 0xFFu)];
        kind = e.x & 0xFF;
    }
    if (kind == 1) return false;
    if (kind == 2) { data_off = e.y; prefix = e.x >> 8; return true; }
    uint32_t node = e.y;
    for (int bi = t.l24 ? 24 : 16; bi < 32; ++bi) {
        const uint2 nd = t.nodes[node];
        const uint32_t rec = ((addr >> (31 - bi)) & 1) ? nd.y : nd.x;
        if (rec == t.node_count) return false;
        if (rec < t.node_count) node = rec;
        else {
            const uint32_t off = rec - t.node_count;
            if (off < 16) return false;  // reference: MmdbError -> lookup error; treated as not found (never produced by builders)
            data_off = off - 16;
            prefix = (uint32_t)bi + 1;   // tree:76-80: depth counts from 96 in v6 trees and 96 is subtracted again
            return true;
        }
    }
    return false;
}
__device__ __forceinline__ bool trie_v4(const DevDb& db, uint32_t addr, uint32_t& data_off, uint32_t& prefix) {
    return trie_v4_tables(IpTables{db.ip_l24, db.ip_l1, db.ip_leaf, db.ip_nodes, db.node_count}, addr, data_off, prefix);
}

// SearchTree::lookup_v6 (tree.rs:92-125): the walk from the root, whatever the tree's version.
__device__ bool trie_v6(const DevDb& db, const uint16_t seg[8], uint32_t& data_off, uint32_t& prefix) {
    uint32_t node = 0;
    for (int bi = 0; bi < 128; ++bi) {
        uint2 nd = db.ip_nodes[node];
        uint32_t bit = (seg[bi >> 4] >> (15 - (bi & 15))) & 1;
        uint32_t rec = bit ? nd.y : nd.x;
        if (rec == db.node_count) return false;
        if (rec < db.node_count) node = rec;
        else {
            uint32_t off = rec - db.node_count;
            if (off < 16) return false;
            data_off = off - 16;
            prefix = (uint32_t)bi + 1;
            return true;
        }
    }
    return false;
}

// One lane's hit -> dense FinalHit record (+ its pattern ids and data offsets), device copy and pinned host mirror: the body of
// k_pack, also called straight from k_lookup for bulk scans (LookupParams::direct), where it overlaps the PCIe writes of
// the records with the lookups instead of running as a kernel of its own afterwards. Wave-uniform call; `valid` marks the
// lanes that hold a hit. Glob ids come from `globs` (k_lookup's own result list) or, when that is null, from pp.ids.
// Pattern results follow Database::lookup_string_uncached (database.rs:911-981): the literal id counts only if it has a data
// mapping, then the glob ids in ascending order; a literal without mapping and no glob is NotFound.
__device__ __forceinline__ void pack_record(const PackParams& pp, bool valid, const Hit& h, const uint32_t* globs) {
    const uint32_t lane = lane_id();
    uint32_t nid = 0, lit_off = 0xFFFFFFFFu;
    if (valid && h.kind == 3) {
        if (h.a != 0xFFFFFFFFu && h.a < pp.n_lit) lit_off = pp.lit_offsets[h.a];
        nid = (lit_off != 0xFFFFFFFFu ? 1u : 0u) + h.n_globs;
        if (nid == 0) valid = false;
    }
    // dense slot for the record: one atomic per wave
    const uint64_t vm = __ballot(valid);
    if (vm == 0) return;
    uint32_t slot0 = 0;
    if (lane == 0) slot0 = atomicAdd(&pp.counters->n_final, (uint32_t)__popcll(vm));
    slot0 = __builtin_amdgcn_readfirstlane(slot0);
    const uint32_t slot = slot0 + (uint32_t)__popcll(vm & lanemask_lt());
    // side-array space for pattern ids: wave exclusive scan of nid, one atomic per wave
    uint32_t scan = valid ? nid : 0u;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)scan, off);
        if ((int)lane >= off) scan += t;
    }
    const uint32_t total = (uint32_t)__shfl((int)scan, 63);
    uint32_t ids0 = 0;
    if (total) {
        if (lane == 0) ids0 = atomicAdd(&pp.counters->n_final_ids, total);
        ids0 = __builtin_amdgcn_readfirstlane(ids0);
    }
    if (valid) {
        const uint32_t my_ids = ids0 + scan - nid;
        FinalHit f{};
        f.start = h.start;
        f.len_type = h.len_type;
        f.kind = h.kind;
        f.prefix_len = h.prefix_len;
        if (h.kind == 2) f.value = h.a;
        else {
            f.n_ids = (uint16_t)nid;
            f.value = my_ids;
            uint32_t w = my_ids;
            if (lit_off != 0xFFFFFFFFu) {
                if (w < pp.out_ids_cap) { pp.out_ids[w] = h.a; pp.out_offs[w] = (long long)lit_off; }
                if (w < pp.host_ids_cap) { pp.host_ids[w] = h.a; pp.host_offs[w] = (long long)lit_off; }
                ++w;
            }
            for (uint32_t k = 0; k < h.n_globs; ++k, ++w) {
                const uint32_t pid = globs ? globs[k] : ((h.ids_off + k < pp.ids_cap) ? pp.ids[h.ids_off + k] : 0u);
                const long long go = pid < pp.n_glob ? (long long)pp.glob_offsets[pid] : -1ll;
                if (w < pp.out_ids_cap) { pp.out_ids[w] = pid; pp.out_offs[w] = go; }
                if (w < pp.host_ids_cap) { pp.host_ids[w] = pid; pp.host_offs[w] = go; }
            }
        }
        if (slot < pp.out_cap) pp.out[slot] = f;
        if (slot < pp.host_cap) pp.host_out[slot] = f;
    }
}

// Rust `<Ipv6Addr as FromStr>` restricted to [0-9A-Fa-f:] input (no embedded IPv4 possible): read_ipv6_addr.
__device__ bool d_parse_ipv6(const uint8_t* s, uint32_t n, uint16_t seg[8]) {
    uint32_t pos = 0;
    uint16_t head[8], tail[7];
    for (int i = 0; i < 8; ++i) head[i] = 0;
    for (int i = 0; i < 7; ++i) tail[i] = 0;
    auto read_groups = [&](uint16_t* g, uint32_t limit) -> uint32_t {
        for (uint32_t i = 0; i < limit; ++i) {
            uint32_t save = pos;
            if (i > 0) {
                if (pos < n && s[pos] == ':') ++pos;
                else { pos = save; return i; }
            }
            uint32_t v = 0, digits = 0, q = pos;
            bool ok = true;
            while (q < n && d_is_hex(s[q])) {
                uint32_t ch = s[q];
                v = v * 16 + (d_is_digit(ch) ? ch - '0' : (ch | 0x20) - 'a' + 10);
                ++digits;
                ++q;
                if (digits > 4) { ok = false; break; }
            }
            if (!ok || digits == 0) { pos = save; return i; }
            g[i] = (uint16_t)v;
            pos = q;
        }
        return limit;
    };
    uint32_t hs = read_groups(head, 8);
    if (hs == 8) {
        if (pos != n) return false;
        for (int i = 0; i < 8; ++i) seg[i] = head[i];
        return true;
    }
    if (!(pos < n && s[pos] == ':')) return false;
    ++pos;
    if (!(pos < n && s[pos] == ':')) return false;
    ++pos;
    uint32_t limit = 8 - (hs + 1);
    uint32_t ts = read_groups(tail, limit);
    if (pos != n) return false;
    for (uint32_t i = 0; i < ts; ++i) head[8 - ts + i] = tail[i];
    for (int i = 0; i < 8; ++i) seg[i] = head[i];
    return true;
}

// One transition of the flattened automaton. States are numbered breadth-first, so the rows of the shallowest states —
// where almost every step of a non-matching text happens — are the first ones; the kernels keep them in LDS.
struct DfaView { const uint8_t* cls; const uint32_t* rows; uint32_t lds_states; };   // cls, rows: LDS
__device__ __forceinline__ uint32_t dfa_step(const DevDb& db, const DfaView& dv, uint32_t st, uint32_t byte) {
    const uint32_t c = dv.cls[byte];
    return st < dv.lds_states ? dv.rows[st * db.dfa_k + c] : db.dfa[(size_t)st * db.dfa_k + c];
}
template <uint32_t ENTRIES>
__device__ __forceinline__ DfaView dfa_stage(const DevDb& db, uint8_t* cls, uint32_t* rows) {   // call before a __syncthreads()
    DfaView dv{cls, rows, 0};
    if (db.dfa) {
        dv.lds_states = min(db.dfa_states, ENTRIES / db.dfa_k);
        for (uint32_t k = threadIdx.x; k < 256; k += blockDim.x) cls[k] = db.dfa_cls[k];
        for (uint32_t k = threadIdx.x, nk = dv.lds_states * db.dfa_k; k < nk; k += blockDim.x) rows[k] = db.dfa[k];
    } else {
        for (uint32_t k = threadIdx.x; k < 256; k += blockDim.x) cls[k] = 0;
    }
    return dv;
}

}  // namespace mxy
