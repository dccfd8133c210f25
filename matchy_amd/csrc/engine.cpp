#include "engine.h"
#include "batch_reader.h"
#include "distinct.h"
#include "extract_render_core.h"
#include "render_core.h"
#include "tally.h"
#include "unicode_lower.h"

#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <unordered_set>

#include "domain_prefilter.h"
#include "hashes.h"

namespace mxy {

void check_launch(const char* kernel) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) throw HipError{std::string("launch of ") + kernel + ": " + hipGetErrorString(e)};
}

// ------------------------------------------------------------------------------------------------ PSL
namespace {

std::string lib_dir() {
    Dl_info info;
    if (dladdr((void*)&lib_dir, &info) && info.dli_fname) {
        std::string p = info.dli_fname;
        size_t s = p.rfind('/');
        if (s != std::string::npos) return p.substr(0, s);
    }
    return ".";
}

bool read_file(const std::string& path, std::vector<uint8_t>& out) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    uint8_t tmp[65536];
    size_t n;
    out.clear();
    while ((n = fread(tmp, 1, sizeof(tmp), f)) > 0) out.insert(out.end(), tmp, tmp + n);
    fclose(f);
    return true;
}

uint32_t tld_hash(const uint8_t* s, size_t n) {  // must match tld_hash_step/tld_hash_bit in device_common.h
    uint32_t h = 2166136261u;
    for (size_t i = 0; i < n; ++i) h = (h ^ s[i]) * 16777619u;
    return (h ^ (h >> 15)) & (TLD_BLOOM_BITS - 1);
}

PslHost* load_psl() {
    std::vector<std::string> candidates;
    if (const char* env = getenv("MATCHY_AMD_PSL")) candidates.push_back(env);
    std::string d = lib_dir();
    candidates.push_back(d + "/../data/psl.bin");
    candidates.push_back(d + "/data/psl.bin");
    candidates.push_back(d + "/psl.bin");
    std::vector<uint8_t> buf;
    bool ok = false;
    for (auto& c : candidates) if (read_file(c, buf)) { ok = true; break; }
    if (!ok) throw std::runtime_error("matchy_amd: cannot find the public-suffix container psl.bin (set MATCHY_AMD_PSL)");
    if (buf.size() < 16 || memcmp(buf.data(), "PSLB", 4) != 0) throw std::runtime_error("matchy_amd: bad psl.bin header");
    uint32_t count, bytes;
    memcpy(&count, &buf[8], 4);
    memcpy(&bytes, &buf[12], 4);
    auto* h = new PslHost();
    std::string prev;
    size_t p = 16;
    for (uint32_t i = 0; i < count; ++i) {
        if (p + 2 > buf.size()) throw std::runtime_error("matchy_amd: truncated psl.bin");
        uint8_t shared = buf[p], rest = buf[p + 1];
        p += 2;
        if (shared > prev.size() || p + rest > buf.size()) throw std::runtime_error("matchy_amd: corrupt psl.bin");
        std::string s = prev.substr(0, shared) + std::string((const char*)&buf[p], rest);
        p += rest;
        h->suffixes.push_back(s);
        prev.swap(s);
    }
    size_t cap = 16;
    while (cap < h->suffixes.size() * 3) cap <<= 1;
    h->mask = (uint32_t)(cap - 1);
    h->slots.assign(cap, PslSlot{0, 0, 0});
    // two filters in one array: [0, TLD_BLOOM_WORDS) over the last labels of all suffixes, byte-wise hash (the general walk of
    // k_validate); behind it TLD_BLOOM_WORDS / 2 words for k_anchor's prefilter — what its 8-byte window shows of a label: the label if it
    // fits, its first 8 bytes if it does not (label_window_keep, domain_prefilter.h) —, TWO bits per key from the two-multiply hash (bits
    // 0..13 and 14..27). (Until round 3 the prefilter folded the first filter, which also held its
    // bits, to half its size: a quarter of all short labels passed, "html" among them.)
    static_assert(TLD_PREFILTER_BITS == TLD_BLOOM_BITS / 2, "the prefilter's filter is the second half of the array");
    h->bloom.assign(TLD_BLOOM_WORDS + TLD_BLOOM_WORDS / 2, 0);
    h->tld_pfx.assign(1u << TLD_PFX_BITS, make_uint2(0u, 0u));
    uint32_t n_pfx = 0;
    for (const std::string& s : h->suffixes) {
        if (s.empty()) continue;
        uint64_t rh = psl_hash_init();
        for (size_t k = s.size(); k-- > 0;) rh = psl_hash_step(rh, (uint8_t)s[k]);
        uint64_t hh = psl_hash_finish(rh);
        uint32_t slot = (uint32_t)hh & h->mask;
        while (h->slots[slot].len != 0) slot = (slot + 1) & h->mask;
        h->slots[slot] = PslSlot{hh, (uint32_t)h->pool.size(), (uint32_t)s.size()};
        h->pool.insert(h->pool.end(), s.begin(), s.end());
        size_t dot = s.rfind('.');
        const uint8_t* last = (const uint8_t*)s.data() + (dot == std::string::npos ? 0 : dot + 1);
        size_t ll = s.size() - (dot == std::string::npos ? 0 : dot + 1);
        uint32_t bit = tld_hash(last, ll);
        h->bloom[bit >> 5] |= 1u << (bit & 31);
        // k_anchor's prefilter: its filter and, for the labels that fill its 8-byte window, the exact table k_validate_dom asks
        if (ll >= 1 && prefilter_add_label(&h->bloom[TLD_BLOOM_WORDS], h->tld_pfx.data(), last, ll) && ++n_pfx > TLD_PFX_MAX_KEYS)
            throw std::runtime_error("matchy_amd: psl.bin has more long last labels than the prefix table holds (TLD_PFX_BITS)");
        h->max_tld_len = std::max<uint32_t>(h->max_tld_len, (uint32_t)ll);
        h->max_suffix_len = std::max<uint32_t>(h->max_suffix_len, (uint32_t)s.size());
        if (ll) h->tld_first[last[0] >> 5] |= 1u << (last[0] & 31);
    }
    // exact table of short last labels; flag 1 = the label by itself is a suffix ("com"), unlike e.g. "ck" (only "*.ck")
    h->tld_tab.assign(1u << TLD_TAB_BITS, make_uint2(0u, 0u));
    std::unordered_set<std::string> whole(h->suffixes.begin(), h->suffixes.end());
    for (const std::string& s : h->suffixes) {
        size_t dot = s.rfind('.');
        std::string l = dot == std::string::npos ? s : s.substr(dot + 1);
        if (l.empty() || l.size() > 7) continue;
        uint8_t k[8] = {0};
        memcpy(k, l.data(), l.size());
        uint32_t lo, hi;
        memcpy(&lo, k, 4);
        memcpy(&hi, k + 4, 4);
        const uint32_t flags = 0x80u | (whole.count(l) ? 1u : 0u);
        uint32_t slot = tld_tab_slot(lo, hi);
        for (;;) {
            uint2& e = h->tld_tab[slot];
            if ((e.y >> 24) == 0) { e = make_uint2(lo, hi | (flags << 24)); break; }
            if (e.x == lo && (e.y & 0xFFFFFFu) == hi) break;  // same label from another suffix
            slot = (slot + 1) & ((1u << TLD_TAB_BITS) - 1);
        }
    }
    return h;
}

}  // namespace

const PslHost& PslHost::get() {
    static PslHost* inst = load_psl();
    return *inst;
}

// ------------------------------------------------------------------------------------------------ device image
void DeviceDb::upload(const DbImage& img, int dev) {
    device = dev;
    MXY_HIP(hipSetDevice(dev));
    const PslHost& psl = PslHost::get();
    std::vector<uint2> nodes;
    uint32_t v4_start;
    img.build_ip_nodes(nodes, v4_start);
    ip_nodes.upload(nodes);
    view.ip_nodes = ip_nodes.p;
    view.node_count = img.node_count;
    view.ip_version = (uint32_t)img.ip_version;
    view.v4_start_node = v4_start;
    view.has_ip = img.has_ip;
    bytes_uploaded = nodes.size() * sizeof(uint2);
    {
        // First-level table for IPv4: the outcome of the first 16 steps of SearchTree::lookup_v4 (tree.rs:46-90) for
        // every 16-bit prefix, so a lookup is one table load plus the (usually 1-3) remaining levels instead of ~18
        // dependent node loads. Entry: x = kind | prefix_len << 8 (kind 0 continue at node y, 1 not found,
        // 2 found with data offset y).
        std::vector<uint2> l1(65536, make_uint2(1u, 0u));
        if (img.node_count > 0) {
            for (uint32_t v = 0; v < 65536; ++v) {
                uint32_t node = v4_start;
                uint2 e = make_uint2(0u, 0u);
                bool done = false;
                for (int bi = 0; bi < 16 && !done; ++bi) {
                    const uint2 nd = nodes[node];
                    const uint32_t rec = ((v >> (15 - bi)) & 1) ? nd.y : nd.x;
                    if (rec == img.node_count) { e = make_uint2(1u, 0u); done = true; }
                    else if (rec < img.node_count) node = rec;
                    else {
                        const uint32_t off = rec - img.node_count;
                        e = off < 16 ? make_uint2(1u, 0u) : make_uint2(2u | ((uint32_t)(bi + 1) << 8), off - 16);
                        done = true;
                    }
                }
                if (!done) e = make_uint2(0u, node);
                l1[v] = e;
            }
        }
        ip_l1.upload(l1);
        view.ip_l1 = ip_l1.p;
        bytes_uploaded += l1.size() * sizeof(uint2);
        // /24 occupancy bitmap (2 MiB): bit v is clear iff lookup_v4 of every address under prefix v ends in "not found"
        // within the first 24 levels. The streaming kernel drops such candidates right after validation (they are still
        // counted), so only addresses that can hit reach the lookups.
        // First 24 levels as a direct table (2^24 entries, 128 MB of the 288 GB), and below a /24 that is not decided yet a LEAF
        // table with the outcome for each of its 256 addresses (2 KB per such /24: 40 K host addresses are 80 MB, 900 K are
        // 1.8 GB — what 288 GB of HBM are for): every IPv4 lookup is two dependent loads instead of 1 + up to 16. Entry kind 3 in
        // the /24 table: y = leaf index. Leaf tables are capped at 16 GB (MATCHY_AMD_LEAF_MB); /24s beyond the cap keep kind 0
        // (continue at node y: the reference's walk). All three are built on the device (ip_tables.hip): one walk per /24 and
        // per leaf address over the tree that was uploaded above. Tiny trees (< 4096 nodes; MATCHY_AMD_L24=0 / 1 forces) do
        // without the 128 MB table: 16-level table + walk, bitmap from the host.
        bool want24 = img.node_count >= 4096;
        if (const char* e = getenv("MATCHY_AMD_L24")) want24 = atoi(e) != 0 && img.node_count > 0;
        std::vector<uint32_t> bm(1u << 19, 0u);
        // The tables are accelerators, not requirements: when their memory cannot be had (a smaller GPU, a process that holds several
        // databases) the open degrades — no leaf tables (undecided /24s continue at their node: the reference's walk), then no /24
        // table at all (16-level table + walk, below) — instead of failing. The leaf tables take at most a quarter of what is free.
        bool have24 = false;
        if (want24) {
            try {
                ip_l24.alloc((size_t)1 << 24);
                ip_bm24.alloc(bm.size());
                DevBuf<uint32_t> ctr;
                ctr.alloc(2);
                MXY_HIP(hipMemset(ctr.p, 0, 8));
                launch_ip_l24(ip_nodes.p, img.node_count, v4_start, ip_l24.p, ip_bm24.p, ctr.p, nullptr);
                uint32_t undecided = 0;
                MXY_HIP(hipMemcpy(&undecided, ctr.p, 4, hipMemcpyDeviceToHost));
                size_t cap_leaf = ((size_t)16 << 30) / (256 * sizeof(uint2));
                size_t mem_free = 0, mem_total = 0;
                if (hipMemGetInfo(&mem_free, &mem_total) == hipSuccess) cap_leaf = std::min(cap_leaf, mem_free / 4 / (256 * sizeof(uint2)));
                else (void)hipGetLastError();
                if (const char* e = getenv("MATCHY_AMD_LEAF_MB")) cap_leaf = ((size_t)atoll(e) << 20) / (256 * sizeof(uint2));
                size_t n_leaf = std::min<size_t>(undecided, cap_leaf);
                DevBuf<uint32_t> leaf_node;
                if (n_leaf) {
                    try {
                        ip_leaf.alloc(n_leaf * 256);
                        leaf_node.alloc(n_leaf);
                    } catch (const HipError&) {
                        (void)hipGetLastError();
                        ip_leaf.free();
                        n_leaf = 0;   // the /24 entries of the undecided prefixes stay "continue at node"
                    }
                }
                if (n_leaf) {
                    launch_ip_leaf(ip_nodes.p, img.node_count, ip_l24.p, ctr.p + 1, (uint32_t)n_leaf, leaf_node.p, ip_leaf.p, nullptr);
                    MXY_HIP(hipDeviceSynchronize());   // leaf_node is released below
                    view.ip_leaf = ip_leaf.p;
                    bytes_uploaded += n_leaf * 256 * sizeof(uint2);
                }
                view.ip_l24 = ip_l24.p;
                bytes_uploaded += ((size_t)1 << 24) * sizeof(uint2);
                MXY_HIP(hipMemcpy(bm.data(), ip_bm24.p, bm.size() * 4, hipMemcpyDeviceToHost));   // for the statistics below
                have24 = true;
            } catch (const HipError&) {
                (void)hipGetLastError();
                ip_l24.free(); ip_leaf.free(); ip_bm24.free();
                view.ip_l24 = nullptr; view.ip_leaf = nullptr;
                std::fill(bm.begin(), bm.end(), 0u);
            }
        }
        if (!have24) {
            if (img.node_count > 0) {
                auto set_range = [&](uint32_t first, uint32_t count) {
                    for (uint32_t v = first; v < first + count;) {
                        if ((v & 31) == 0 && v + 32 <= first + count) { bm[v >> 5] = 0xFFFFFFFFu; v += 32; }
                        else { bm[v >> 5] |= 1u << (v & 31); ++v; }
                    }
                };
                struct Frame { uint32_t node, prefix, depth; };
                std::vector<Frame> st;
                st.push_back({v4_start, 0u, 0u});
                while (!st.empty()) {
                    const Frame f = st.back();
                    st.pop_back();
                    const uint2 nd = nodes[f.node];
                    for (uint32_t bit = 0; bit < 2; ++bit) {
                        const uint32_t rec = bit ? nd.y : nd.x;
                        const uint32_t depth = f.depth + 1;                       // levels consumed
                        const uint32_t prefix = f.prefix | (bit << (24 - depth));  // left-aligned in 24 bits
                        if (rec == img.node_count) continue;
                        if (rec < img.node_count) {
                            if (depth == 24) set_range(prefix, 1);
                            else st.push_back({rec, prefix, depth});
                        } else if (rec - img.node_count >= 16) {
                            set_range(prefix, 1u << (24 - depth));
                        }
                    }
                }
            }
            ip_bm24.upload(bm);
        }
        view.ip_bm24 = ip_bm24.p;
        {
            uint64_t set = 0;
            for (uint32_t wv : bm) set += (uint64_t)__builtin_popcount(wv);
            view.ip_bm24_permille = (uint32_t)(set * 1000 / ((uint64_t)bm.size() * 32));
            view.ip_bm24_any = set ? 1u : 0u;
        }
        bytes_uploaded += bm.size() * 4;
    }
    if (img.has_literal) {
        std::vector<LitSlot> slots;
        uint32_t mask;
        img.build_lit_table(slots, mask);
        lit_slots.upload(slots);
        const uint8_t* pool = img.bytes.data() + img.lh_off + img.lh_strings_offset;
        std::vector<uint8_t> pv(pool, pool + img.lh_strings_size);
        lit_pool.upload(pv);
        {
            // >= 64 bits per literal (false-positive rate <= 1.6 %), at least 4 Mbit: L2-resident for typical databases
            size_t bits = (size_t)1 << 22;
            size_t live = 0;
            for (const LitSlot& sl : slots) live += sl.str_off != 0xFFFFFFFFu;
            while (bits < live * 64 && bits < ((size_t)1 << 31)) bits <<= 1;
            std::vector<uint32_t> bm(bits / 32, 0u);
            const uint32_t bmask = (uint32_t)(bits - 1);
            // names of <= 31 bytes are tested whole (k_validate_dom decides names that fit its 32-byte context; longer ones take
            // the general path, which lists every valid name); keys of 32 bytes and more — file hashes — enter with their first 32
            // bytes and their length (k_validate tests every hex token of a hash length that way before it lists it)
            for (const LitSlot& sl : slots) {
                if (sl.str_off == 0xFFFFFFFFu || (size_t)sl.str_off + 2 > pv.size()) continue;
                const size_t kl = (size_t)pv[sl.str_off] | ((size_t)pv[sl.str_off + 1] << 8);
                if ((size_t)sl.str_off + 2 + kl > pv.size()) continue;
                uint64_t lane[4] = {0, 0, 0, 0};
                memcpy(lane, pv.data() + sl.str_off + 2, std::min<size_t>(kl, 32));
                const uint32_t b = name_hash31(lane[0], lane[1], lane[2], lane[3], (uint32_t)kl) & bmask;
                bm[b >> 5] |= 1u << (b & 31);
            }
            lit_bm.upload(bm);
            view.lit_bm = lit_bm.p; view.lit_bm_mask = bmask;
            bytes_uploaded += bm.size() * 4;
        }
        // longest stored key: a query that is longer after lower-casing cannot match any literal
        uint32_t max_len = 0;
        for (const LitSlot& sl : slots)
            if (sl.str_off != 0xFFFFFFFFu && (size_t)sl.str_off + 2 <= pv.size()) max_len = std::max<uint32_t>(max_len, (uint32_t)pv[sl.str_off] | ((uint32_t)pv[sl.str_off + 1] << 8));
        view.lit_max_len = max_len;
        view.lit_slots = lit_slots.p; view.lit_mask = mask; view.has_literal = 1;
        view.lit_pool = lit_pool.p; view.lit_pool_size = img.lh_strings_size;
        bytes_uploaded += slots.size() * sizeof(LitSlot) + pv.size();
    }
    if (img.has_glob) {
        const uint8_t* pgp = img.bytes.data() + img.pg_off;
        std::vector<uint8_t> pv(pgp, pgp + img.pg_len);
        pv.resize((pv.size() + 3) & ~(size_t)3, 0);
        pg.upload(pv);
        std::vector<uint32_t> off, ids;
        img.build_lit2pat(off, ids);
        if (ids.empty()) ids.push_back(0);
        lit2pat_off.upload(off);
        lit2pat.upload(ids);
        auto r32 = [&](size_t o) { uint32_t v; memcpy(&v, pgp + o, 4); return v; };
        view.pg = pg.p; view.pg_len = (uint32_t)img.pg_len; view.has_glob = 1;
        view.ac_start = r32(20); view.ac_size = r32(24);
        view.patterns_off = r32(36); view.pattern_count = r32(32);
        uint32_t unaligned = r32(40) + r32(44);
        view.wild_off = unaligned + (8 - unaligned % 8) % 8;  // recomputed like the reader (pg:1089-1093)
        view.wild_count = r32(60);
        view.glob_seg_off = r32(104);
        view.glob_max_segs = 1;
        for (uint32_t pid = 0; pid < view.pattern_count; ++pid) view.glob_max_segs = std::max<uint32_t>(view.glob_max_segs, r32((size_t)view.glob_seg_off + (size_t)pid * 8 + 4) & 0xFFFFu);
        view.lit2pat_off = lit2pat_off.p; view.lit2pat = lit2pat.p; view.n_ac_lits = (uint32_t)off.size() - 1;
        {
            // one dependent load per text byte instead of a node + edge-list walk with failure links: the automaton as a
            // dense table in HBM (there is room: a million literals need a few GB)
            std::vector<uint32_t> nx, noff;
            std::vector<uint8_t> cls;
            uint32_t k = 0;
            size_t limit = (size_t)8 << 30;
            if (const char* env = getenv("MATCHY_AMD_DFA_MAX_MB")) limit = (size_t)atoll(env) << 20;
            bool alnum_literal = true;
            view.ac_alnum = 1;
            if (img.build_ac_dfa(nx, cls, k, noff, limit, &alnum_literal)) {
                view.ac_alnum = alnum_literal ? 1u : 0u;
                // case-insensitive: the automaton holds lower-cased literals and the text is ASCII-lower-cased while it is
                // walked (paraglob_offset.rs:1198-1206) — here by giving 'A'..'Z' the classes of 'a'..'z'
                if (img.match_mode == 1) for (int c = 'A'; c <= 'Z'; ++c) cls[c] = cls[c + 32];
                dfa.upload(nx); dfa_node.upload(noff); dfa_cls.upload(cls);
                view.dfa = dfa.p; view.dfa_node = dfa_node.p; view.dfa_cls = dfa_cls.p; view.dfa_k = k;
                view.dfa_states = (uint32_t)noff.size();
                bytes_uploaded += nx.size() * 4 + noff.size() * 4 + 256;
            }
        }
        bytes_uploaded += pv.size() + (off.size() + ids.size()) * 4;
        // Suffix filter (DevDb::sfx_bm): every pattern is star + literal of >= 3 bytes (shorter ones can never match: they get no
        // automaton literal, Q8), all literals begin with the same byte, at most 4 different counts of that byte per literal.
        if (view.dfa && view.wild_count == 0 && view.pattern_count && !getenv("MATCHY_AMD_NO_SUFFIX_FILTER")) {
            const bool ci_db = img.match_mode == 1;
            bool ok = true;
            int first = -1;
            uint32_t dots = 0;
            std::vector<std::pair<uint32_t, uint32_t>> lits;   // (offset, length) in the paraglob buffer
            for (uint32_t pid = 0; pid < view.pattern_count && ok; ++pid) {
                const size_t io = (size_t)view.glob_seg_off + (size_t)pid * 8;
                const uint32_t firsth = r32(io), count = r32(io + 4) & 0xFFFFu;
                if (count != 2 || (size_t)firsth + 24 > img.pg_len) { ok = false; break; }
                const uint8_t* h0 = pgp + firsth;
                const uint8_t* h1 = pgp + firsth + 12;
                uint32_t dlen, doff;
                memcpy(&dlen, h1 + 4, 4); memcpy(&doff, h1 + 8, 4);
                if (h0[0] != 1 || h1[0] != 0 || (size_t)doff + dlen > img.pg_len) { ok = false; break; }
                if (dlen < 3) continue;   // never matches
                const uint8_t* l = pgp + doff;
                const int fb = ci_db ? (int)ascii_lower1(l[0]) : (int)l[0];
                if (first < 0) first = fb;
                if (fb != first) { ok = false; break; }
                uint32_t d = 0;
                for (uint32_t k = 0; k < dlen; ++k) d += (ci_db ? ascii_lower1(l[k]) : l[k]) == (uint32_t)first;
                if (d > 32) { ok = false; break; }
                dots |= 1u << (d - 1);
                if (dlen <= 31) lits.push_back({doff, dlen});   // a longer literal cannot end a name of <= 31 bytes (the ones decided here)
            }
            if (ok && first >= 0 && __builtin_popcount(dots) <= 4) {
                size_t bits = (size_t)1 << 16;
                while (bits < lits.size() * 64 && bits < ((size_t)1 << 31)) bits <<= 1;
                std::vector<uint32_t> bm(bits / 32, 0u);
                const uint32_t bmask = (uint32_t)(bits - 1);
                for (auto& ol : lits) {
                    uint64_t lane[4] = {0, 0, 0, 0};
                    memcpy(lane, pgp + ol.first, ol.second);
                    if (ci_db) for (uint64_t& w : lane) w = ascii_lower8(w);
                    const uint32_t b = name_hash31(lane[0], lane[1], lane[2], lane[3], ol.second) & bmask;
                    bm[b >> 5] |= 1u << (b & 31);
                }
                sfx_bm.upload(bm);
                view.sfx_bm = sfx_bm.p; view.sfx_mask = bmask; view.sfx_first = (uint32_t)first; view.sfx_dots = dots;
                bytes_uploaded += bm.size() * 4;
            }
        }
    }
    view.ci = img.match_mode == 1 ? 1u : 0u;
    if (view.ci) {
        const LowerTable& lt = LowerTable::get();
        std::vector<uint32_t> m;
        m.reserve(lt.map.size() * 3);
        for (const LowerMapEntry& e : lt.map) {
            m.push_back(e.cp);
            m.push_back((uint32_t)e.len | ((uint32_t)e.utf8[0] << 8) | ((uint32_t)e.utf8[1] << 16) | ((uint32_t)e.utf8[2] << 24));
            m.push_back((uint32_t)e.utf8[3] | ((uint32_t)e.utf8[4] << 8) | ((uint32_t)e.utf8[5] << 16) | ((uint32_t)e.utf8[6] << 24));
        }
        std::vector<uint2> ri, rc;
        for (const CpRange& r : lt.ignorable) ri.push_back(make_uint2(r.first, r.last));
        for (const CpRange& r : lt.cased) rc.push_back(make_uint2(r.first, r.last));
        lc_map.upload(m); lc_ign.upload(ri); lc_cased.upload(rc);
        view.lc_map = lc_map.p; view.lc_n = (uint32_t)lt.map.size();
        view.lc_ign = lc_ign.p; view.lc_n_ign = (uint32_t)ri.size();
        view.lc_cased = lc_cased.p; view.lc_n_cased = (uint32_t)rc.size();
        bytes_uploaded += m.size() * 4 + (ri.size() + rc.size()) * 8;
    }
    {
        // pattern id -> data offset tables for pack_record
        std::vector<uint32_t> lo, go;
        if (img.has_literal) {
            if (!img.lit_data_offsets.empty()) lo = img.lit_data_offsets;
            else {
                uint32_t mx = 0;
                for (auto& kv : img.lit_data_map) mx = std::max(mx, kv.first + 1);
                lo.assign(mx, 0xFFFFFFFFu);
                for (auto& kv : img.lit_data_map) lo[kv.first] = kv.second;
            }
        }
        if (img.has_glob) {
            go.resize(img.pdm_count);
            if (img.pdm_count) memcpy(go.data(), img.bytes.data() + img.pdm_off, img.pdm_count * 4);
        }
        if (lo.empty()) lo.push_back(0xFFFFFFFFu);
        if (go.empty()) go.push_back(0);
        n_lit_offsets = img.has_literal ? (uint32_t)lo.size() : 0;
        n_glob_offsets = img.has_glob ? (uint32_t)img.pdm_count : 0;
        lit_offsets.upload(lo);
        glob_offsets.upload(go);
    }
    psl_slots.upload(psl.slots);
    psl_pool.upload(psl.pool);
    bloom.upload(psl.bloom);
    view.psl_slots = psl_slots.p; view.psl_mask = psl.mask; view.psl_pool = psl_pool.p; view.tld_bloom = bloom.p;
    view.max_tld_len = psl.max_tld_len;
    view.max_suffix_len = psl.max_suffix_len;
    tld_tab.upload(psl.tld_tab);
    view.tld_tab = tld_tab.p;
    tld_pfx.upload(psl.tld_pfx);
    view.tld_pfx = tld_pfx.p;
    for (int k = 0; k < 8; ++k) view.tld_first[k] = psl.tld_first[k];
    bytes_uploaded += psl.slots.size() * sizeof(PslSlot) + psl.pool.size() + psl.bloom.size() * 4;
}

// ------------------------------------------------------------------------------------------------ scanner
Scanner::Scanner(std::shared_ptr<const DbImage> img, std::shared_ptr<DeviceDb> ddb, uint32_t extract_flags, uint32_t min_labels)
    : img_(std::move(img)), ddb_(std::move(ddb)), flags_(extract_flags), min_labels_(min_labels ? min_labels : 2) {
    MXY_HIP(hipSetDevice(ddb_->device));
    hipDeviceProp_t prop;
    MXY_HIP(hipGetDeviceProperties(&prop, ddb_->device));
    n_cu_ = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    counters_.alloc(MAX_SLICES);
    MXY_HIP(hipMemset(counters_.p, 0, sizeof(ScanCounters) * MAX_SLICES));
    counters_clean_ = true;
    host_slices_.alloc(MAX_SLICES);
    for (Event& e : ev_) e.create();
    ev_fork_.create(hipEventDisableTiming);
    ev_join_.create(hipEventDisableTiming);
    aux_stream_.create(hipStreamNonBlocking);
    ev_join2_.create(hipEventDisableTiming);
    aux2_stream_.create(hipStreamNonBlocking);
}

Scanner::~Scanner() = default;   // here: DistinctSet and HitTally are incomplete in the header

void Scanner::set_unique(bool on) {
    if (on && !distinct_) {
        distinct_ = std::make_unique<DistinctSet>();
        // MATCHY_AMD_TRACE: fetch prints the device time of the dedup kernels beside the extraction kernels' of the same batch
        if (getenv("MATCHY_AMD_TRACE")) { distinct_->set_profile(true); profile_ = true; }
    }
    unique_ = on;
}
void Scanner::reset_unique() {
    if (!distinct_) return;
    MXY_HIP(hipSetDevice(ddb_->device));
    distinct_->reset();
}
uint64_t Scanner::unique_count() const { return distinct_ ? distinct_->count() : 0; }

void Scanner::set_tally(bool on) {
    if (on && !tally_) tally_ = std::make_unique<HitTally>();
    tally_on_ = on;
}
void Scanner::reset_tally() {
    if (!tally_) return;
    MXY_HIP(hipSetDevice(ddb_->device));
    tally_->reset();
}
void Scanner::tally_top(size_t limit, std::vector<TallyEntry>& out) {
    out.clear();
    if (!tally_) return;
    MXY_HIP(hipSetDevice(ddb_->device));
    tally_->top(limit, out, nullptr);   // the null stream: every add() ended with its scan's stream synchronised, nothing is in flight
}

// work lists of one slice for `len` bytes of log
void Scanner::Work::ensure(uint32_t len) {
    const size_t want_c = std::max<size_t>(4096, (size_t)len / 24);
    const size_t want_r = std::max<size_t>(1024, (size_t)len / 256);
    const size_t want_h = std::max<size_t>(1024, want_c / 4);
    if (cands.n < want_c) cands.alloc(want_c);
    if (hits.n < want_h) hits.alloc(want_h);
    if (ids.n < want_h) ids.alloc(want_h);
    if (cands_a.n < want_c) cands_a.alloc(want_c);
    if (cands_m.n < want_c / 8) cands_m.alloc(want_c / 8);
    if (cands_r.n < want_r) cands_r.alloc(want_r);
    if (cands_d.n < want_r) cands_d.alloc(want_r);
    if (rare.n < want_r) rare.alloc(want_r);
    if (rare_dom.n < want_r) rare_dom.alloc(want_r);
    if (tok.n < want_r) tok.alloc(want_r);
    if (heavy.n < want_r) heavy.alloc(want_r);
    // domain anchor list: slots of DOM_PLANES dwords, whole 1024-slot chunks (see TokParams::dom_list)
    const size_t want_d = ((std::max<size_t>(8192, (size_t)len / 96) + ANCHOR_CHUNK - 1) / ANCHOR_CHUNK) * ANCHOR_CHUNK;
    if (dom_slots < want_d) { dom_list.alloc(want_d * DOM_PLANES); dom_slots = want_d; }
}

void Scanner::ensure_final(size_t recs, size_t ids) {
    if (final_.n < recs) final_.alloc(recs);
    if (final_ids_.n < recs + ids) { final_ids_.alloc(recs + ids); final_offs_.alloc(recs + ids); }
}

void Scanner::ensure_capacity(uint32_t len) {
    work_[0].ensure(len);
    ensure_final(work_[0].hits.n, work_[0].ids.n);
}

static_assert(sizeof(FinalHit) == ResultLayout::REC_BYTES, "result_layout.h lays out FinalHit records");

namespace {
// the three arrays of a result block (result_layout.h) that begins at `block`
struct ResultArrays { FinalHit* recs; uint32_t* ids; long long* offs; };
ResultArrays arrays_of(uint8_t* block, const ResultLayout& l) {
    return {(FinalHit*)block, (uint32_t*)(block + l.ids_offset()), (long long*)(block + l.offs_offset())};
}
}  // namespace

// Neither capacity shrinks. The layout is recorded when the block exists: a failed allocation leaves an empty mirror of no capacity.
void Scanner::ensure_mirror(uint32_t recs, uint32_t ids) {
    if (mirror_.p && mirror_layout_.recs_cap >= recs && mirror_layout_.ids_cap >= ids) return;
    const ResultLayout want{std::max<size_t>(recs, mirror_layout_.recs_cap), std::max<size_t>(ids, mirror_layout_.ids_cap)};
    mirror_layout_ = ResultLayout{};
    mirror_.alloc(want.bytes());
    mirror_layout_ = want;
}

namespace {
// grid multipliers (workgroups per CU) of k_anchor / k_validate_dom / k_lookup: what is resident at once (grid-stride kernels; a
// larger grid only adds a partially filled second round).
// k_anchor: one full round of resident workgroups; k_validate_dom: one; k_lookup: 2 per CU measured best (the string
// lookups are chains of dependent loads: more waves in flight only add contention on the random table accesses).
void grid_multipliers(bool filter_ac, int (&gm)[3]) {
    static const int occ_a = anchor_blocks_per_cu(), occ_v = validate_blocks_per_cu(false), occ_v_ac = validate_blocks_per_cu(true);
    // k_validate_dom: at most 4 workgroups per CU — the fifth that registers and LDS would allow leaves no LDS for the kernels
    // that run beside it (k_validate over tokens / IPv6 / e-mail anchors: 26 KB per workgroup), which then start when
    // k_validate_dom's workgroups retire (measured: tail 0.250 -> 0.232 ms)
    gm[0] = occ_a; gm[1] = std::min(filter_ac ? occ_v_ac : occ_v, 4); gm[2] = 2;
    for (int& m : gm) m = std::max(1, std::min(m, 64));
}
}  // namespace

// workgroups for a list kernel: the default while the previous scan's list was short, else one workgroup per `per_wg` entries of it,
// at most max_per_cu per CU (workgroups beyond the end of a list leave at once)
int Scanner::grid_for(uint32_t n_hint, uint32_t per_wg, int dflt, int max_per_cu) const {
    const uint64_t want = ((uint64_t)n_hint + per_wg - 1) / per_wg;
    return (int)std::max<uint64_t>((uint64_t)dflt, std::min<uint64_t>(want, (uint64_t)n_cu_ * (uint64_t)max_per_cu));
}

namespace {
size_t grown_list(uint32_t n) { return (size_t)n + n / 4 + 1024; }   // a list regrown for a demand of n entries
// point the parameters of a kernel at the candidate list `l` of a slice and at the counter `n` of its entries
void point_at(TokParams& t, const DevBuf<Candidate>& l, uint32_t* n) { t.cands = l.p; t.cand_cap = (uint32_t)l.n; t.n_cand = n; }
void point_at(LookupParams& p, const DevBuf<Candidate>& l, const uint32_t* n) { p.cands = l.p; p.cand_cap = (uint32_t)l.n; p.n_in = n; }
}  // namespace

// Kernel parameters of slice `sl` for the byte range [lo, hi) of the batch (hi = len + 1 for the range that ends the batch).
// The lists and counters are the slice's own; the final record arrays (and the counters that hand out their slots: slice 0's)
// are shared by all slices.
void Scanner::slice_params(int sl, const ScanRequest& rq, uint32_t lo, uint32_t hi, SliceLaunch& L) {
    const uint8_t* dptr = rq.ptr;
    const uint32_t len = rq.len;
    const bool lookup = rq.lookup;
    Work& w = work_[sl];
    ScanCounters* ctr = counters_.p + sl;
    TokParams& tp = L.tp;
    tp = TokParams{};
    tp.log = dptr; tp.len = len; tp.flags = flags_; tp.min_labels = min_labels_;
    tp.filter_v4 = lookup ? 1u : 0u;
    // without a glob section a string candidate can only hit through the literal table
    // with a glob section also through a glob, and every glob with a literal part needs an output state of the AC
    // automaton on the way (pure-wildcard patterns match without one: no prefilter then)
    const bool ac_ok = ddb_->view.has_glob && ddb_->view.dfa && ddb_->view.wild_count == 0;
    tp.filter_ac = (lookup && ac_ok) ? 1u : 0u;
    tp.filter_lit = (lookup && (!ddb_->view.has_glob || ac_ok)) ? 1u : 0u;
    if (const char* dbg = getenv("MATCHY_AMD_DEBUG")) tp.debug = (uint32_t)atoi(dbg);
    point_at(tp, w.cands, &ctr->n_cand);
    tp.cands_a = w.cands_a.p; tp.cand_a_cap = (uint32_t)w.cands_a.n;
    // IPv4 candidates are listed sparsely when the /24 bitmap of the database filters most of the address space
    tp.cand_chunk = (lookup && ddb_->view.ip_bm24_permille <= 250) ? 64u : 1024u;
    tp.rare = w.rare.p; tp.rare_cap = (uint32_t)w.rare.n;
    tp.rare_dom = w.rare_dom.p; tp.rare_dom_cap = (uint32_t)w.rare_dom.n;
    tp.vmode = 7u;
    tp.tok = w.tok.p; tp.tok_cap = (uint32_t)w.tok.n;
    tp.heavy = w.heavy.p; tp.heavy_cap = (uint32_t)w.heavy.n;
    tp.dom_list = w.dom_list.p; tp.dom_cap = (uint32_t)w.dom_slots;
    tp.counters = ctr;
    grid_multipliers(tp.filter_ac != 0, L.gm);
    {
        // k_anchor: one round of resident workgroups and ONE segment per wave, all of the same size — the segments are
        // handed out statically, so anything else leaves some waves with one segment more than the others (with three or
        // four segments per wave that was 19 % of the kernel), and every segment end flushes the wave's anchor rings.
        // Short ranges get SEG_MIN segments and fewer waves.
        const uint64_t waves = (uint64_t)n_cu_ * L.gm[0] * 4;
        const uint64_t span = (uint64_t)hi - lo;
        const uint64_t sb = ((span + waves - 1) / waves + SEG_ALIGN - 1) / SEG_ALIGN * SEG_ALIGN;
        tp.seg_bytes = (uint32_t)std::min<uint64_t>(SEG_MAX, std::max<uint64_t>(SEG_MIN, sb));
        tp.n_segs = (uint32_t)((span + tp.seg_bytes - 1) / tp.seg_bytes);
        tp.seg_base = lo; tp.scan_end = hi;
    }
    L.grid_anchor = (int)std::min<uint32_t>((tp.n_segs + 3) / 4, (uint32_t)n_cu_ * L.gm[0]);
    if (L.grid_anchor < 1) L.grid_anchor = 1;
    {
        // starting chunk of k_anchor's sparse lists when the previous batch filled them (SparseWriter in k_anchor.hip): a quarter of what a
        // wave wrote then, in whole 64-slot steps, at most 4032 (the chunk state holds 12 bits)
        const uint32_t waves = (uint32_t)L.grid_anchor * 4u;
        auto chunk_for = [&](uint32_t n_prev) -> uint32_t {
            if (n_prev < 262144u) return 0u;
            return std::min<uint32_t>(4032u, std::max<uint32_t>(64u, (n_prev / waves / 4u) & ~63u));
        };
        tp.tok_chunk = chunk_for(hint_.n_tok);
        tp.rare_chunk = chunk_for(hint_.n_rare);
    }
    LookupParams& lp = L.lp;
    lp = LookupParams{};
    if (lookup) {
        lp.log = dptr; lp.len = len; lp.cands = w.cands.p; lp.cand_cap = (uint32_t)w.cands.n;
        lp.hits = w.hits.p; lp.hit_cap = (uint32_t)w.hits.n; lp.ids = w.ids.p; lp.ids_cap = (uint32_t)w.ids.n;
        if (ddb_->view.has_glob) {
            if (w.glob_work.n < w.cands.n / 8) w.glob_work.alloc(w.cands.n / 8);
            lp.glob_work = w.glob_work.p; lp.glob_work_cap = (uint32_t)w.glob_work.n;
            if (early_glob_ && sl == 0 && ac_ok) {
                if (w.glob_work_d.n < w.cands.n / 8) w.glob_work_d.alloc(w.cands.n / 8);
                tp.glob_work_d = w.glob_work_d.p; tp.glob_work_d_cap = (uint32_t)w.glob_work_d.n;
                lp.early_glob = 1u;
            }
            setup_spill(sl, lp);
        }
        lp.counters = ctr;
        PackParams pp{};
        pp.hits = w.hits.p; pp.hit_cap = (uint32_t)w.hits.n; pp.ids = w.ids.p; pp.ids_cap = (uint32_t)w.ids.n;
        pp.lit_offsets = ddb_->lit_offsets.p; pp.n_lit = ddb_->n_lit_offsets;
        pp.glob_offsets = ddb_->glob_offsets.p; pp.n_glob = ddb_->n_glob_offsets;
        pp.out = final_.p; pp.out_cap = (uint32_t)final_.n;
        pp.out_ids = final_ids_.p; pp.out_offs = final_offs_.p; pp.out_ids_cap = (uint32_t)final_ids_.n;
        if (rq.host_mirror) {
            const ResultArrays m = arrays_of(mirror_.p, mirror_layout_);
            pp.host_out = m.recs; pp.host_cap = (uint32_t)mirror_layout_.recs_cap;
            pp.host_ids = m.ids; pp.host_offs = m.offs;
            pp.host_ids_cap = (uint32_t)mirror_layout_.ids_cap;
        }
        if (compact_) {
            pp.c4_out = c4_.p; pp.c4_cap = (uint32_t)c4_.n;
            if (rq.host_mirror) { pp.host_c4 = mirror_c4_.p; pp.host_c4_cap = (uint32_t)mirror_c4_.n; }
        }
        pp.counters = counters_.p;   // n_final / n_final_ids of slice 0 hand out the slots of the shared record arrays
        // k_lookup writes the final records itself (the PCIe writes of the mirror overlap the lookups); only the
        // single-query path (lookup_one) reads the raw hit list
        lp.direct = 1u;
        lp.pk = pp;
        // sparse IPv4 candidates (the /24 bitmap lets a few per cent through): k_anchor looks them up itself while it streams
        // (k_anchor.hip v4_lookup_flush) — their hit records, most of the result traffic of a log scan, then cross the bus under
        // the streaming pass instead of behind it. Dense lists (a database that answers most addresses) keep the lookup kernel:
        // there the walks are the work, and a kernel of lanes that do nothing else hides their latency better.
        tp.inline_v4 = (tp.filter_v4 && tp.cand_chunk == 64u) ? 1u : 0u;
        tp.pk = pp;
    }
    // a database without any IPv4 answer lists no IPv4 candidate (the /24 bitmap is empty): nothing to look up
    L.ip_pass = lookup && !tp.inline_v4 && (ddb_->view.ip_bm24_any || !tp.filter_v4);
    L.la = lp;
    if (L.ip_pass) {
        point_at(L.la, w.cands_a, &ctr->n_cand_a);
        L.la.glob_work = nullptr; L.la.glob_work_cap = 0;
    }
    // Forked scans of a database without globs: the third stream (tokens, IPv6 / e-mail anchors, k_rare) gets a candidate list and a
    // lookup pass of its own, so the scan's stream does not have to join it in front of its lookups (an event wait between two
    // kernels costs ~20 us of the chain even when the event is long done). With a glob section the lookups share the glob work
    // list and its counter: one list, joined as before.
    L.split_misc = lookup && !ddb_->view.has_glob;
    L.lm = lp;
    L.lr = lp;
    L.ld = lp;
    if (lp.early_glob) {
        // forked scan of a glob database: the undecided domains get a list and ONE glob pass over all of it (no work list: a few thousand
        // candidates) on a stream of their own; what spills there is listed with bit 31 set and read from cands_alt by the spill pass
        lp.cands_alt = w.cands_d.p; lp.cand_alt_cap = (uint32_t)w.cands_d.n;
        L.ld = lp;
        point_at(L.ld, w.cands_d, &ctr->n_cand_d);
        L.ld.glob_work = nullptr; L.ld.glob_work_cap = 0; L.ld.early_glob = 0; L.ld.spill_tag = 1u;
    }
    if (L.split_misc) {
        point_at(L.ld, w.cands_d, &ctr->n_cand_d);
        point_at(L.lm, w.cands_m, &ctr->n_cand_m);
        point_at(L.lr, w.cands_r, &ctr->n_cand_r);
    }
    // one workgroup on every other CU: enough lanes to keep the result traffic on the bus, and the validation kernels beside it
    // keep nearly all of their resident waves (128 / 256 / 512 workgroups measured 1.199 / 1.213 / 1.241 ms per headline batch)
    // (dense lists — a database that answers most addresses, C5 — are latency-bound trie walks for every line: full grid)
    L.ip_dense = tp.cand_chunk != 64u;
    L.ip_grid = L.ip_dense ? n_cu_ * L.gm[2] : std::max(1, n_cu_ / 2);
}

// How a device-resident batch of `len` bytes is cut into `want` equal slices (matchy_scanner_set_slices: tests, experiments):
// cuts[0] = 0 < cuts[1] < ... < cuts[n] = len + 1, inner cuts on SEG_ALIGN boundaries. The default (want = 0) is ONE slice: measured
// on the headline batch (profiles/r03_slices_sweep.txt), with k_anchor's segments handed out statically — one per resident wave —
// the tail kernels of slice i take wave slots that k_anchor of slice i + 1 needs at its start, the workgroups that start late finish
// late, and the whole scan gets slower (2 slices 1.32 ms, 4 slices 1.53 ms against 1.16 ms for one).
int Scanner::plan_slices(uint32_t len, int want, uint32_t (&cuts)[MAX_SLICES + 1]) {
    cuts[0] = 0;
    cuts[1] = len + 1;
    if (want <= 0) return 1;
    const uint64_t unit = SEG_ALIGN;
    // a slice wants at least one segment
    const int n = (int)std::min<uint64_t>((uint64_t)std::min(want, (int)MAX_SLICES), std::max<uint64_t>(1, ((uint64_t)len + 1) / unit));
    for (int k = 1; k < n; ++k) {
        uint64_t c = (uint64_t)((double)len * k / n) / unit * unit;
        c = std::max<uint64_t>(c, (uint64_t)cuts[k - 1] + unit);
        cuts[k] = (uint32_t)c;
    }
    cuts[n] = len + 1;
    for (int k = 1; k <= n; ++k) if (cuts[k] <= cuts[k - 1]) return (cuts[1] = len + 1, 1);   // degenerate: one slice
    return n;
}

void Scanner::scan_device(const ScanRequest& rq, hipStream_t stream) {
    if (rq.len >= 0x7FFF0000u) throw HipError{"scan_device: chunk too large (must be < 2^31 bytes)"};
    if (((uintptr_t)rq.ptr & 15) != 0) throw HipError{"scan_device: device pointer must be 16-byte aligned"};
    MXY_HIP(hipSetDevice(ddb_->device));
    last_ = rq;
    compact_ = rq.compact && rq.lookup && compact_possible();
    last_forked_ = false;
    spill_done_ = false;
    expect_chains_ = 0;
    if (rq.whole_lines) { launch_whole_lines(rq, stream); return; }
    // MATCHY_AMD_NO_FORK=1 keeps everything on one stream.
    static const bool env_no_fork = getenv("MATCHY_AMD_NO_FORK") != nullptr;
    const bool no_fork = env_no_fork || !rq.fork;
    uint32_t cuts[MAX_SLICES + 1] = {0, rq.len + 1};
    const int ns = (no_fork || !rq.lookup) ? 1 : plan_slices(rq.len, rq.slices, cuts);
    n_slices_ = ns;
    // buffers first: what they may allocate (lists, mirror, glob work list) must not sit between the launches
    if (ns == 1) ensure_capacity(rq.len);
    else {
        size_t recs = 0, ids = 0;
        for (int k = 0; k < ns; ++k) { work_[k].ensure(cuts[k + 1] - cuts[k]); recs += work_[k].hits.n; ids += work_[k].ids.n; }
        ensure_final(recs, ids);
    }
    mirror_used_ = false;
    if (rq.lookup && rq.host_mirror) {
        static const uint32_t mirror0 = getenv("MATCHY_AMD_MIRROR_RECS") ? (uint32_t)atoi(getenv("MATCHY_AMD_MIRROR_RECS")) : (1u << 20);
        ensure_mirror(std::max(mirror0, 16u), std::max(mirror0 / 16, 16u));
        if (compact_) mirror_c4_.ensure(std::max(mirror0, 16u));
        mirror_used_ = true;
    }
    if (compact_ && c4_.n < final_.n) c4_.alloc(final_.n);
    // databases with globs, one slice, forked: k_validate_dom queues the candidates it flags for the glob pass itself
    early_glob_ = !no_fork && ns == 1 && rq.lookup && ddb_->view.has_glob;
    for (int k = 0; k < ns; ++k) slice_params(k, rq, cuts[k], cuts[k + 1], launch_[k]);
    early_glob_ = early_glob_ && launch_[0].lp.early_glob != 0;
    // the counter blocks are zero already when the last scan ended with fetch() (k_finish copies them out and clears them)
    if (!counters_clean_) { MXY_HIP(hipMemsetAsync(counters_.p, 0, sizeof(ScanCounters) * MAX_SLICES, stream)); dom_preset_ = 0; }
    counters_clean_ = false;
    {
        // First chunks of the domain list without a reservation (DomWriter::reserve): when the previous batch needed more than one chunk per
        // wave on average, wave w of k_anchor owns chunk w and the counter starts behind those chunks — k_finish of the previous scan has
        // written that value already when the batches are alike; otherwise it is set here.
        const uint64_t total = (uint64_t)launch_[0].grid_anchor * 4u * ANCHOR_CHUNK;
        uint32_t want = 0;
        if (ns == 1 && total <= launch_[0].tp.dom_cap && (uint64_t)hint_.n_dom * 2 >= total * 3) want = (uint32_t)total;
        if (want != dom_preset_) MXY_HIP(hipMemsetD32Async((hipDeviceptr_t)&counters_.p->n_dom, (int)want, 1, stream));
        dom_preset_ = want;
        dom_want_ = want;
        launch_[0].tp.dom_static = want ? ANCHOR_CHUNK : 0u;
        // behind the first chunk: an eighth of what a wave wrote last time, in whole tiles, 256..ANCHOR_CHUNK slots (less padding for k_validate_dom
        // to read; these reservations are spread over the kernel)
        for (int k = 0; k < ns; ++k) launch_[k].tp.dom_chunk = ANCHOR_CHUNK;
        if (want) {
            const uint32_t share = hint_.n_dom / ((uint32_t)launch_[0].grid_anchor * 4u) / 8u;
            launch_[0].tp.dom_chunk = std::min<uint32_t>(ANCHOR_CHUNK, std::max<uint32_t>(256u, share & ~63u));
        }
    }
    if (profile_) MXY_HIP(hipEventRecord(ev_[0], stream));
    if (ns > 1) launch_sliced(ns, stream);
    else if (no_fork) launch_one_stream(stream);
    else launch_forked(stream);
    if (profile_) MXY_HIP(hipEventRecord(ev_[4], stream));
}

void Scanner::ensure_dom_stream() {
    if (dom_stream_) return;
    dom_stream_.create(hipStreamNonBlocking);
    ev_join3_.create(hipEventDisableTiming);
    ev_dom_.create(hipEventDisableTiming);
}

// Sliced scan. The scan's stream carries the k_anchor launches, slice after slice. Behind k_anchor of slice i three side streams
// take over, as in the one-slice fork (launch_forked): dom_stream_ k_validate_dom -> k_validate (undecided domains) -> k_lookup;
// aux_stream_ k_lookup_ip; aux2_stream_ k_validate (tokens, IPv6 / e-mail) -> k_rare. They run BESIDE k_anchor of slice i + 1
// (whose workgroups leave the CUs one by one), the slices of one side stream in stream order. Only the tail of the last slice is
// not covered by a k_anchor.
void Scanner::launch_sliced(int ns, hipStream_t stream) {
    const DevDb& view = ddb_->view;
    last_forked_ = true;
    ensure_dom_stream();
    for (Event& e : ev_anchor_) e.create(hipEventDisableTiming);
    for (Event& e : ev_misc_) e.create(hipEventDisableTiming);
    for (int k = 0; k < ns; ++k) {
        SliceLaunch& L = launch_[k];
        ScanCounters* ctr = counters_.p + k;
        launch_anchor(L.tp, view, L.grid_anchor, stream);
        hipEvent_t done = ev_anchor_[k];
        if (profile_ && k == ns - 1) { MXY_HIP(hipEventRecord(ev_[1], stream)); done = ev_[1]; }
        else MXY_HIP(hipEventRecord(done, stream));
        if (L.ip_pass) {
            MXY_HIP(hipStreamWaitEvent(aux_stream_, done, 0));
            launch_lookup_ip(L.la, view, L.ip_grid, L.ip_dense, aux_stream_);
        }
        MXY_HIP(hipStreamWaitEvent(aux2_stream_, done, 0));
        TokParams t1 = L.tp;
        t1.vmode = 5u;
        if (L.split_misc) point_at(t1, work_[k].cands_m, &ctr->n_cand_m);
        launch_validate_misc(t1, view, std::max(1, n_cu_ / 2), aux2_stream_);
        if (L.split_misc) launch_lookup(L.lm, view, std::max(1, n_cu_ / 2), aux2_stream_);
        if (rare_possible()) {
            TokParams tr = t1;
            tr.vmode = L.tp.vmode;
            if (L.split_misc) point_at(tr, work_[k].cands_r, &ctr->n_cand_r);
            launch_rare(tr, view, n_cu_ * 4, aux2_stream_);
            if (L.split_misc) launch_lookup(L.lr, view, std::max(1, n_cu_ / 8), aux2_stream_);
        }
        MXY_HIP(hipEventRecord(ev_misc_[k], aux2_stream_));
        MXY_HIP(hipStreamWaitEvent(dom_stream_, done, 0));
        launch_validate_dom(L.tp, view, n_cu_ * L.gm[1], dom_stream_);
        TokParams t2 = L.tp;
        t2.vmode = 2u;
        launch_validate_misc(t2, view, n_cu_, dom_stream_);
        if (!L.split_misc) MXY_HIP(hipStreamWaitEvent(dom_stream_, ev_misc_[k], 0));
        launch_lookup(L.lp, view, n_cu_ * L.gm[2], dom_stream_);
    }
    MXY_HIP(hipEventRecord(ev_join3_, dom_stream_));
    MXY_HIP(hipStreamWaitEvent(stream, ev_join3_, 0));
    if (launch_[0].split_misc) MXY_HIP(hipStreamWaitEvent(stream, ev_misc_[ns - 1], 0));
    bool any_ip = false;
    for (int k = 0; k < ns; ++k) any_ip |= launch_[k].ip_pass;
    if (any_ip) {
        MXY_HIP(hipEventRecord(ev_join_, aux_stream_));
        MXY_HIP(hipStreamWaitEvent(stream, ev_join_, 0));
    }
}

// One slice forked after k_anchor. Everything k_anchor lists is complete then, and two parts of the rest do not depend on
// k_validate_dom:
//  * the trie lookups of the IPv4 candidates (and the PCIe writes of their hit records, which is most of the result traffic
//    of a log scan) -> k_lookup_ip on a stream of its own; both lookup passes append to the same final arrays (atomic slot
//    reservation);
//  * k_validate over the long tokens and k_anchor's IPv6 / e-mail anchors, and k_rare behind it -> a third stream.
// The scan's stream keeps k_validate_dom, k_validate over the domain anchors k_validate_dom left undecided, and the lookups
// of the validation kernels' candidates; it joins the third stream before those lookups and the second after them.
void Scanner::launch_forked(hipStream_t stream) {
    SliceLaunch& L = launch_[0];
    const TokParams& tp = L.tp;
    const DevDb& view = ddb_->view;
    Work& w = work_[0];
    ScanCounters* ctr = counters_.p;
    launch_anchor(tp, view, L.grid_anchor, stream);
    if (profile_) MXY_HIP(hipEventRecord(ev_[1], stream));
    last_forked_ = true;
    hipEvent_t fork = profile_ ? ev_[1] : ev_fork_;
    if (!profile_) MXY_HIP(hipEventRecord(ev_fork_, stream));
    if (L.ip_pass) {
        MXY_HIP(hipStreamWaitEvent(aux_stream_, fork, 0));
        launch_lookup_ip(L.la, view, L.ip_grid, L.ip_dense, aux_stream_);
        MXY_HIP(hipEventRecord(ev_join_, aux_stream_));
    }
    MXY_HIP(hipStreamWaitEvent(aux2_stream_, fork, 0));
    TokParams t1 = tp;
    t1.vmode = 5u;
    if (L.split_misc) point_at(t1, w.cands_m, &ctr->n_cand_m);
    // split lists: the lookups of k_validate's candidates do not wait for k_rare (checksum validators: a chain of their own,
    // almost always over next to nothing), whose few candidates get a list and a lookup launch of their own — on the second
    // stream when the IPv4 lookups do not need it (they run inside k_anchor), beside the third stream's lookups. The long tokens
    // — k_rare takes what they leave — then get a launch of their own in front of the rare anchors (IPv6 / e-mail: ten times as
    // many, 0.12 ms), so that k_rare runs beside those instead of behind them.
    const bool rare_own = L.split_misc && rare_possible() && !L.ip_pass;
    // Long lists (dense logs): these passes wait for memory most of their time, and beyond a few workgroups per CU more of them only
    // queue up in front of it. Measured per pass on 1.85 GB batches (profiles/r05_log_shapes.txt): long tokens 8 -> 6 per CU: step
    // 2.61 -> 2.41 ms (endpoint log with hashes); '@' / "::" anchors 8 -> 4: 2.37 -> 2.31 (JSON lines); domains k_validate_dom left
    // undecided 8 -> 2: 2.36 -> 2.22 (proxy log with URLs). Short lists keep their default grids.
    constexpr int TOK_WGS_PER_CU = 6, RARE_WGS_PER_CU = 4, RARE_DOM_WGS_PER_CU = 2;
    // Both lists long (the previous batch had hundreds of thousands of long tokens AND of IPv6 / e-mail anchors: application logs in
    // JSON lines): the long tokens do not run in front of the rare anchors on the third stream but beside them on the second, in front
    // of k_rare (which takes what they leave: stream order instead of an event), and list their hashes in k_rare's candidate list — the
    // lookup behind k_rare takes both. Two latency-bound passes over millions of entries each then overlap instead of queueing (the
    // JSON-lines shape: tail 1.18 -> see profiles/r04_log_shapes.txt). With short lists (a web-server log) the two kernels would only
    // take vector-ALU time from k_validate_dom beside them (+6 us measured): the order stays as it is there.
    static const int env_tok_aside = getenv("MATCHY_AMD_TOK_ASIDE") ? atoi(getenv("MATCHY_AMD_TOK_ASIDE")) : -1;
    const bool tok_aside = rare_own && (env_tok_aside >= 0 ? env_tok_aside != 0 : (hint_.n_tok >= 262144u && hint_.n_rare >= 262144u));
    const int tok_grid = grid_for(hint_.n_tok, 1024, std::max(1, n_cu_ / 2), TOK_WGS_PER_CU);   // 6 KB of LDS, workgroups beyond the list leave at once
    if (tok_aside) {
        MXY_HIP(hipStreamWaitEvent(aux_stream_, fork, 0));
        TokParams tt = t1;
        tt.vmode = 4u;
        point_at(tt, w.cands_r, &ctr->n_cand_r);
        launch_validate_misc(tt, view, tok_grid, aux_stream_);
        t1.vmode = 1u;
    } else if (rare_own) {
        TokParams tt = t1;
        tt.vmode = 4u;
        launch_validate_misc(tt, view, tok_grid, aux2_stream_);
        ev_v1_.create(hipEventDisableTiming);
        MXY_HIP(hipEventRecord(ev_v1_, aux2_stream_));
        t1.vmode = 1u;
    }
    // beside k_validate_dom: half the CUs, so that kernel keeps most of its resident waves (more when the previous batch's lists were long)
    launch_validate_misc(t1, view, grid_for(rare_own ? hint_.n_rare : std::max(hint_.n_rare, hint_.n_tok), 1024, std::max(1, n_cu_ / 2), rare_own ? RARE_WGS_PER_CU : 8), aux2_stream_);
    // Split lists: the side chains do not join the scan's stream through events — the last kernel of each (a k_lookup launch) reports
    // its end in ScanCounters::chains_done, which k_finish polls (arrive_chain 1: third stream, 2: k_rare's, 3: the fourth stream)
    uint32_t chains = 0;
    if (L.split_misc) {
        LookupParams lm = L.lm;
        if (rare_own || !rare_possible()) { lm.arrive_chain = 1; lm.arrive = ctr; ++chains; }
        launch_lookup(lm, view, grid_for(hint_.n_cand_m, 512, std::max(1, n_cu_ / 2), 4), aux2_stream_);
    }
    if (rare_possible()) {   // one wave per SIMD (297 VGPRs)
        TokParams tr = t1;
        tr.vmode = tp.vmode;
        if (L.split_misc) point_at(tr, w.cands_r, &ctr->n_cand_r);
        hipStream_t rs = rare_own ? aux_stream_ : aux2_stream_;
        if (rare_own && !tok_aside) MXY_HIP(hipStreamWaitEvent(aux_stream_, ev_v1_, 0));
        launch_rare(tr, view, grid_for(hint_.n_heavy, 128, n_cu_ * 4, 16), rs);
        if (L.split_misc) {
            LookupParams lr = L.lr;
            lr.arrive_chain = rare_own ? 2u : 1u; lr.arrive = ctr; ++chains;
            launch_lookup(lr, view, grid_for(hint_.n_cand_r, 512, std::max(1, n_cu_ / 8), 4), rs);   // (tok_aside: the hint follows the list that now holds the hashes too)
        }
    }
    if (!L.split_misc) MXY_HIP(hipEventRecord(ev_join2_, aux2_stream_));
    launch_validate_dom(tp, view, n_cu_ * L.gm[1], stream);
    TokParams t2 = tp;
    t2.vmode = 2u;
    if (L.split_misc) {
        // Behind k_validate_dom two chains: the few domain anchors it left undecided (general walk + lookups of THEIR candidates,
        // a list of their own) stay on the scan's stream — no event between producer and consumer —, the lookups of
        // k_validate_dom's candidates go to a fourth stream beside them and report their end to k_finish like the other side chains.
        ensure_dom_stream();
        MXY_HIP(hipEventRecord(ev_dom_, stream));
        MXY_HIP(hipStreamWaitEvent(dom_stream_, ev_dom_, 0));
        LookupParams lpm = L.lp;
        lpm.arrive_chain = 3; lpm.arrive = ctr; ++chains;
        // one workgroup per CU: every workgroup ends with a pair of returning atomics on the two record counters, and with 512
        // of them those queue up behind each other (64 / 128 / 192 / 256 / 512 workgroups: tail 0.236 / 0.218 / 0.217 / 0.218 / 0.227 ms;
        // not fewer than one per CU: a database that most names hit makes this the kernel with the work)
        launch_lookup(lpm, view, grid_for(hint_.n_cand, 512, n_cu_, 4), dom_stream_);
        expect_chains_ = chains;
        point_at(t2, w.cands_d, &ctr->n_cand_d);
        launch_validate_misc(t2, view, grid_for(hint_.n_rare_dom, 512, n_cu_, RARE_DOM_WGS_PER_CU), stream);
        launch_lookup(L.ld, view, grid_for(hint_.n_cand_d, 512, std::max(1, n_cu_ / 8), 4), stream);
    } else {
        // k_validate<2> and the glob pass over ITS candidates go to the second stream when the early glob pass runs and the IPv4
        // lookups do not need that stream: the lean pass does not have to wait for them
        const bool v2_aside = early_glob_ && !L.ip_pass;
        if (early_glob_) {
            // Databases with globs keep one candidate list, but the candidates k_validate_dom flags for the glob pass — most of that
            // pass's work — are on a work list of their own already (TokParams::glob_work_d): the glob pass over them starts here, on the
            // fourth stream, beside k_validate<2> and the lean pass over everything else (which skips them and defers what IT finds to
            // the usual work list for a second, small glob pass behind it).
            ensure_dom_stream();
            MXY_HIP(hipEventRecord(ev_dom_, stream));
            MXY_HIP(hipStreamWaitEvent(dom_stream_, ev_dom_, 0));
            // Both side chains report their ends to k_finish (arrival counters, as in the scans without globs: an event join in front of
            // k_finish costs ~10-20 us each).
            LookupParams lg = L.lp;
            lg.glob_work = w.glob_work_d.p; lg.glob_work_cap = (uint32_t)w.glob_work_d.n;
            lg.n_work = &ctr->n_glob_work_d;
            lg.arrive_chain = 3; lg.arrive = ctr; ++chains;
            launch_lookup_early_glob(lg, view, n_cu_ * L.gm[2], dom_stream_);
            if (v2_aside) {
                MXY_HIP(hipStreamWaitEvent(aux_stream_, ev_dom_, 0));
                point_at(t2, w.cands_d, &ctr->n_cand_d);
                launch_validate_misc(t2, view, grid_for(hint_.n_rare_dom, 512, n_cu_, 8), aux_stream_);
                LookupParams ld = L.ld;
                ld.arrive_chain = 2; ld.arrive = ctr; ++chains;
                launch_lookup(ld, view, grid_for(hint_.n_cand_d, 512, std::max(2, n_cu_ / 8), 4), aux_stream_);
            }
            expect_chains_ = chains;
        }
        if (!v2_aside) launch_validate_misc(t2, view, grid_for(hint_.n_rare_dom, 512, n_cu_, RARE_DOM_WGS_PER_CU), stream);
        // no timing events inside the forked tail: every packet between two kernels of the chain is ~6-8 us of it, and with
        // kernels running side by side the intervals would not be kernel times anyway (ScanTiming: validate_ms = the whole tail)
        MXY_HIP(hipStreamWaitEvent(stream, ev_join2_, 0));
        if (last_.lookup) launch_lookup(L.lp, view, n_cu_ * L.gm[2], stream);
    }
    if (L.ip_pass) MXY_HIP(hipStreamWaitEvent(stream, ev_join_, 0));
}

// Everything on the scan's stream (MATCHY_AMD_NO_FORK, submit / wait, scan_host).
void Scanner::launch_one_stream(hipStream_t stream) {
    const SliceLaunch& L = launch_[0];
    const TokParams& tp = L.tp;
    const DevDb& view = ddb_->view;
    launch_anchor(tp, view, L.grid_anchor, stream);
    if (profile_) MXY_HIP(hipEventRecord(ev_[1], stream));
    launch_validate_dom(tp, view, n_cu_ * L.gm[1], stream);
    launch_validate_misc(tp, view, grid_for(std::max(std::max(hint_.n_tok, hint_.n_rare), hint_.n_rare_dom), 1024, n_cu_, 8), stream);   // vmode 7: every list
    if (profile_) MXY_HIP(hipEventRecord(ev_[2], stream));
    if (rare_possible()) launch_rare(tp, view, grid_for(hint_.n_heavy, 128, n_cu_ * 4, 16), stream);
    if (profile_) MXY_HIP(hipEventRecord(ev_[3], stream));
    if (last_.lookup) {
        if (L.ip_pass) launch_lookup_ip(L.la, view, L.ip_grid, L.ip_dense, stream);
        launch_lookup(L.lp, view, n_cu_ * L.gm[2], stream);
    }
}

// Whole-line mode (whole_lines.hip): count + prefix, scatter + classify, then the lookup passes over the candidate list — query k is
// candidate k — all on the scan's stream. A list of addresses has a line every ~13 bytes and every line may hit: the candidate list
// (and with it the arrays of the front end, the glob work list and the record arrays) is sized at len / 8 or for the lines of the
// previous batch; a list that is still too short is counted past and regrown by fetch() like every other list.
void Scanner::launch_whole_lines(const ScanRequest& rq, hipStream_t stream) {
    if (!rq.lookup) throw ParamError{"whole-line mode needs a lookup scan"};
    n_slices_ = 1;
    early_glob_ = false;
    if (!wl_) wl_ = std::make_unique<WholeLines>();
    WholeLines& q = *wl_;
    Work& w = work_[0];
    w.ensure(rq.len);
    const size_t want = std::max<size_t>(std::max<size_t>(4096, (size_t)rq.len / 8), grown_list(hint_.n_cand));
    if (w.cands.n < want) w.cands.alloc(want);
    if (w.hits.n < w.cands.n / 4) w.hits.alloc(w.cands.n / 4);   // each_list counts the hit list at a quarter of the candidates
    if (ddb_->view.has_glob && w.glob_work.n < w.cands.n) w.glob_work.alloc(w.cands.n);   // string queries reach the glob pass unwalked
    ensure_final(std::max(w.hits.n, w.cands.n), w.ids.n);
    const uint32_t cap = (uint32_t)std::min<size_t>(w.cands.n, 0x7FFFFFFFu);
    const uint32_t tiles = line_tiles(rq.len), chunks = line_chunks(tiles);
    if (q.counts.n < tiles || !q.prefix.p) { q.counts.alloc((size_t)tiles + tiles / 4 + 1024); q.prefix.alloc(q.counts.n + 1); }
    if (q.chunks.n < chunks) q.chunks.alloc((size_t)chunks + 64);
    if (q.ends.n < cap) { q.ends.alloc(cap); q.invalid.alloc(cap); }
    if (!q.ctr.p) { q.ctr.alloc(1); q.host.alloc(1); }
    mirror_used_ = false;
    if (rq.host_mirror) {
        static const uint32_t mirror0 = getenv("MATCHY_AMD_MIRROR_RECS") ? (uint32_t)atoi(getenv("MATCHY_AMD_MIRROR_RECS")) : (1u << 20);
        ensure_mirror(std::max(mirror0, 16u), std::max(mirror0 / 16, 16u));
        if (compact_) mirror_c4_.ensure(std::max(mirror0, 16u));
        mirror_used_ = true;
    }
    if (compact_ && c4_.n < final_.n) c4_.alloc(final_.n);
    slice_params(0, rq, 0, rq.len + 1, launch_[0]);   // the lookup parameters; the extraction kernels' are not used
    if (!counters_clean_) { MXY_HIP(hipMemsetAsync(counters_.p, 0, sizeof(ScanCounters) * MAX_SLICES, stream)); dom_preset_ = 0; }
    counters_clean_ = false;
    if (dom_preset_) MXY_HIP(hipMemsetD32Async((hipDeviceptr_t)&counters_.p->n_dom, 0, 1, stream));
    dom_preset_ = 0; dom_want_ = 0;
    WholeLineParams p{};
    p.data = rq.ptr; p.len = rq.len; p.prefix = q.prefix.p; p.ends = q.ends.p; p.invalid = q.invalid.p;
    p.cands = w.cands.p; p.cap = cap; p.wl = q.ctr.p; p.counters = counters_.p; p.pk = launch_[0].lp.pk;
    MXY_HIP(hipMemsetAsync(q.invalid.p, 0, std::min<size_t>(cap, (size_t)rq.len + 1), stream));   // a batch has at most len lines
    MXY_HIP(hipMemsetAsync(q.ctr.p, 0, sizeof(WholeLineCounters), stream));
    if (profile_) MXY_HIP(hipEventRecord(ev_[0], stream));
    MXY_HIP(line_index_build(rq.ptr, rq.len, q.counts.p, q.chunks.p, q.prefix.p, n_cu_, stream, nullptr));
    if (profile_) MXY_HIP(hipEventRecord(ev_[1], stream));
    launch_whole_lines_scatter(p, n_cu_, stream);
    launch_whole_lines_classify(p, ddb_->view, n_cu_, stream);
    if (profile_) { MXY_HIP(hipEventRecord(ev_[2], stream)); MXY_HIP(hipEventRecord(ev_[3], stream)); }
    launch_lookup(launch_[0].lp, ddb_->view, n_cu_ * launch_[0].gm[2], stream);
    MXY_HIP(hipMemcpyAsync(q.host.p, q.ctr.p, sizeof(WholeLineCounters), hipMemcpyDeviceToHost, stream));
    if (profile_) MXY_HIP(hipEventRecord(ev_[4], stream));
}

void Scanner::arm_whole_lines(ScanRequest& rq, bool gz) {
    rq.whole_lines = false;
    if (!whole_lines_ || !rq.lookup) return;
    const char* other = gz ? "gz scans" : (segments_ && segments_->pending()) ? "segments" : hit_lines_on_ ? "hit lines" : render_pending_ ? "rendered records" : nullptr;
    if (other) {
        set_segments(nullptr, 0);
        set_render(nullptr);
        throw ParamError{std::string("whole-line mode and ") + other + " cannot be combined"};
    }
    rq.whole_lines = true;
}

size_t sort_hits_temp_bytes(uint32_t n);
hipError_t sort_hits(const FinalHit* fin, uint32_t n, unsigned long long* keys, uint32_t* vals, void* temp, size_t temp_bytes, FinalHit* out,
                     hipStream_t stream);

namespace {
size_t grown(uint32_t n) { return grown_list(n); }
}  // namespace

// Every work list of slice `w` with the counter of its entries in `s`: f(name, capacity, count, grow), grow() reallocates the list for
// the count. glob_work and spill count only while allocated, glob_work_d only with the early glob pass; the domain list is counted in
// slots and allocated in planes; hits holds at least a quarter of the candidate list (visited behind it: its regrow counts).
template <class F>
void Scanner::each_list(Work& w, const ScanCounters& s, F&& f) {
    auto list = [&](const char* name, auto& b, uint32_t n) { f(name, b.n, n, [&b, n] { b.alloc(grown(n)); }); };
    list("cands", w.cands, s.n_cand); list("cands_a", w.cands_a, s.n_cand_a); list("cands_m", w.cands_m, s.n_cand_m);
    list("cands_r", w.cands_r, s.n_cand_r); list("cands_d", w.cands_d, s.n_cand_d);
    list("rare", w.rare, s.n_rare); list("rare_dom", w.rare_dom, s.n_rare_dom); list("tok", w.tok, s.n_tok); list("heavy", w.heavy, s.n_heavy);
    if (w.glob_work.n) list("glob_work", w.glob_work, s.n_glob_work);
    if (early_glob_) list("glob_work_d", w.glob_work_d, s.n_glob_work_d);
    if (w.spill.n) list("spill", w.spill, s.n_spill);
    f("dom_list", w.dom_slots, s.n_dom, [&] {
        w.dom_slots = (((size_t)s.n_dom + s.n_dom / 4 + ANCHOR_CHUNK) / ANCHOR_CHUNK) * ANCHOR_CHUNK;
        w.dom_list.alloc(w.dom_slots * DOM_PLANES);
    });
    f("hits", w.hits.n, std::max<size_t>(s.n_hits, w.cands.n / 4), [&] { w.hits.alloc(std::max<size_t>(grown(s.n_hits), w.cands.n / 4)); });
    list("ids", w.ids, s.n_ids);
}

// Wait for the stream. poll: the scan behind it is about a millisecond (device-resident input), and the runtime's blocking wait
// takes ~10 us longer to notice the end — poll the stream for the first milliseconds, then block. Host-buffer scans wait for tens
// of milliseconds of copies with other threads busy in the runtime (the command line's reader and second scanner): they block.
static void wait_stream(hipStream_t stream, bool poll) {
    if (poll) {
        const auto t0 = std::chrono::steady_clock::now();
        for (;;) {
            const hipError_t e = hipStreamQuery(stream);
            if (e == hipSuccess) return;
            if (e != hipErrorNotReady) throw HipError{std::string("hipStreamQuery: ") + hipGetErrorString(e)};
            if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(4)) break;
        }
    }
    MXY_HIP(hipStreamSynchronize(stream));
}

// The counters of the last scan_device, settled: k_finish copies the counter blocks out, a list that was over is regrown and the scan runs
// again, candidates the glob pass could not hold go through the spill pass. Leaves host_counters_ (and the slices' blocks) final and
// the device counters clean.
void Scanner::settle_counters(bool trace, hipStream_t stream) {
    const int ns = n_slices_;
    // `attempt` counts the regrows of this fetch. While a list is over, its consumers see min(counter, capacity) entries and everything
    // downstream of it under-counts; the most upstream list that is over has an exact count (nothing in front of it was cut), so every
    // regrow settles at least one more stage of the chain for good. The longest chain of lists is dom_list -> rare_dom -> cands_d ->
    // glob_work -> spill -> ids -> final_ids_ -> c4_ (the other roads are shorter): a scan whose kernels count right needs at most
    // MAX_REGROWS regrows, and one that is still over after that many is a miscount, not a dense batch. The spill pass reads the
    // counters again without regrowing anything and is not counted.
    constexpr int MAX_REGROWS = 8;
    for (int attempt = 0;;) {
        // k_finish: the counter blocks go to pinned host memory and are cleared on the device for the next scan
        launch_finish(counters_.p, host_slices_.p, ns, expect_chains_, dom_want_, stream);
        // side chains that report to k_finish end behind the last event scan_device recorded: the interval ends behind k_finish then
        if (profile_ && expect_chains_) MXY_HIP(hipEventRecord(ev_[4], stream));
        expect_chains_ = 0;   // a rescan sets it again; the spill pass below runs on this stream
        wait_stream(stream, last_.fork);
        if (host_slices_.p[0].error & 8u) {
            // k_finish gave up polling for the side chains (they are slow, not lost): the counters it copied are a snapshot and the
            // device copies were left alone. Join the side streams here, then take the counters again without a poll.
            counters_clean_ = false;
            if (trace) fprintf(stderr, "[matchy_amd] k_finish gave up polling for the side chains: joining the side streams on the host\n");
            if (aux_stream_) MXY_HIP(hipStreamSynchronize(aux_stream_));
            if (aux2_stream_) MXY_HIP(hipStreamSynchronize(aux2_stream_));
            if (dom_stream_) MXY_HIP(hipStreamSynchronize(dom_stream_));
            launch_finish(counters_.p, host_slices_.p, ns, 0u, dom_want_, stream);
            wait_stream(stream, false);
        }
        counters_clean_ = true;
        // slice 0 holds n_final / n_final_ids of all slices; statistics are summed
        ScanCounters& c = host_counters_;
        c = host_slices_.p[0];
        for (int k = 1; k < ns; ++k) {
            const ScanCounters& s = host_slices_.p[k];
            c.lines += s.lines; c.cand_true += s.cand_true; c.hits_true += s.hits_true; c.error |= s.error;
        }
        bool over = false;
        std::string over_names;   // trace only: " <list> <demand>><capacity>" of every list that is over (slice k > 0: "<list>[k]")
        auto test = [&](const char* name, int k, size_t cap, size_t need) {
            if (need <= cap) return;
            over = true;
            if (!trace) return;
            char b[96];
            if (k) snprintf(b, sizeof b, " %s[%d] %zu>%zu", name, k, need, cap);
            else snprintf(b, sizeof b, " %s %zu>%zu", name, need, cap);
            over_names += b;
        };
        for (int k = 0; k < ns; ++k)
            each_list(work_[k], host_slices_.p[k], [&](const char* name, size_t cap, size_t need, auto&&) { test(name, k, cap, need); });
        test("final_", 0, final_.n, c.n_final);
        test("final_ids_", 0, final_ids_.n, c.n_final_ids);
        if (compact_) test("c4_", 0, c4_.n, c.n_c4);
        if (!over) {
            // candidates the glob pass could not hold (more results / deeper star nesting than a lane stores): normally none.
            // If there are, the spill pass runs now — its scratch (one bit per pattern id per thread) is allocated only here — and
            // appends their records to the same arrays; the counters are read again afterwards.
            uint32_t n_spill = 0;
            for (int k = 0; k < ns; ++k) n_spill += work_[k].spill.n ? host_slices_.p[k].n_spill : 0u;
            if (n_spill == 0 || spill_done_ || !last_.lookup) break;
            const uint32_t threads = spill_threads();
            const size_t words = launch_[0].lp.spill_words;
            if (spill_scratch_.n < words * SPILL_BLOCKS * threads) spill_scratch_.alloc(words * SPILL_BLOCKS * threads);
            // the spill pass appends to the lists the counters describe: put them back (k_finish cleared them)
            MXY_HIP(hipMemcpyAsync(counters_.p, host_slices_.p, sizeof(ScanCounters) * ns, hipMemcpyHostToDevice, stream));
            counters_clean_ = false;
            for (int k = 0; k < ns; ++k) {
                if (!work_[k].spill.n || !host_slices_.p[k].n_spill) continue;
                LookupParams lp = launch_[k].lp;
                lp.spill_scratch = spill_scratch_.p;
                launch_lookup_spill(lp, ddb_->view, stream);
            }
            spill_done_ = true;
            if (trace) fprintf(stderr, "[matchy_amd] %u candidates to the spill pass\n", n_spill);
            continue;
        }
        if (trace) fprintf(stderr, "[matchy_amd] work buffers overflow (attempt %d): regrow and rescan:%s\n", attempt, over_names.c_str());
        if (single_) throw HipError{"lookup_one: work buffers overflow"};
        if (attempt >= MAX_REGROWS) throw HipError{"scan: work buffers still overflow after regrowing"};
        ++attempt;
        // grow and run again: the kernels count past the capacity without writing, so the counts are exact demands
        size_t recs = 0, ids = 0;
        for (int k = 0; k < ns; ++k) {
            each_list(work_[k], host_slices_.p[k], [](const char*, size_t cap, size_t need, auto&& grow) { if (need > cap) grow(); });
            recs += work_[k].hits.n; ids += work_[k].ids.n;
        }
        if (final_.n < recs || c.n_final > final_.n) final_.alloc(std::max<size_t>(recs, grown(c.n_final)));
        if (final_ids_.n < recs + ids || c.n_final_ids > final_ids_.n) {
            const size_t want = std::max<size_t>(recs + ids, grown(c.n_final_ids));
            final_ids_.alloc(want); final_offs_.alloc(want);
        }
        if (compact_ && c.n_c4 > c4_.n) c4_.alloc(grown(c.n_c4));
        scan_device(last_, stream);
    }
}

// What the settled counters say: the grid hints of the next scan, the error words, the trace line, `out`'s counters, the timings.
void Scanner::report_counters(ScanOutput& out, bool trace) {
    const int ns = n_slices_;
    {
        ListHint hh;
        for (int k = 0; k < ns; ++k) {
            const ScanCounters& q = host_slices_.p[k];
            hh.n_tok = std::max(hh.n_tok, q.n_tok); hh.n_rare = std::max(hh.n_rare, q.n_rare); hh.n_rare_dom = std::max(hh.n_rare_dom, q.n_rare_dom);
            hh.n_heavy = std::max(hh.n_heavy, q.n_heavy); hh.n_cand = std::max(hh.n_cand, q.n_cand); hh.n_cand_m = std::max(hh.n_cand_m, q.n_cand_m);
            hh.n_cand_r = std::max(hh.n_cand_r, q.n_cand_r); hh.n_cand_d = std::max(hh.n_cand_d, q.n_cand_d);
            hh.n_dom = std::max(hh.n_dom, q.n_dom);
        }
        hint_ = hh;
    }
    const ScanCounters& c = host_counters_;
    if (c.error & 1) throw HipError{"scan: a candidate matches more than 65535 glob patterns (the hit record counts pattern ids in 16 bits)"};
    if (c.error & 4) throw HipError{"scan: a candidate is longer than 16 MiB (24-bit length field)"};
    if (trace) {
        ScanCounters t = host_slices_.p[0];
        for (int k = 1; k < ns; ++k) {
            const ScanCounters& s = host_slices_.p[k];
            t.n_dom += s.n_dom; t.n_rare += s.n_rare; t.n_rare_dom += s.n_rare_dom; t.n_tok += s.n_tok; t.n_heavy += s.n_heavy; t.n_cand_a += s.n_cand_a;
            t.n_cand += s.n_cand; t.n_hits += s.n_hits; t.n_ids += s.n_ids; t.n_glob_work += s.n_glob_work;
        }
        fprintf(stderr, "[matchy_amd] slices=%d lines=%llu n_dom=%u n_rare=%u+%u n_tok=%u n_heavy=%u n_cand=%u+%u (true %u) n_hits=%u (true %u) n_ids=%u glob_work=%u final=%u\n",
                ns, c.lines, t.n_dom, t.n_rare, t.n_rare_dom, t.n_tok, t.n_heavy, t.n_cand_a, t.n_cand, c.cand_true, t.n_hits, c.hits_true, t.n_ids, t.n_glob_work, c.n_final);
    }
    out.lines = c.lines; out.n_cand = single_ ? c.n_cand : c.cand_true;
    out.n_hits = !last_.lookup ? 0 : (single_ ? c.hits_true : c.n_final + (compact_ ? c.n_c4 : 0u));
    if (profile_) {
        MXY_HIP(hipEventElapsedTime(&timing_.anchor_ms, ev_[0], ev_[1]));
        if (last_forked_) {   // one interval for everything behind k_anchor (kernels on three streams)
            MXY_HIP(hipEventElapsedTime(&timing_.validate_ms, ev_[1], ev_[4]));
            timing_.rare_ms = 0; timing_.lookup_ms = 0;
        } else {
            MXY_HIP(hipEventElapsedTime(&timing_.validate_ms, ev_[1], ev_[2]));
            MXY_HIP(hipEventElapsedTime(&timing_.rare_ms, ev_[2], ev_[3]));
            MXY_HIP(hipEventElapsedTime(&timing_.lookup_ms, ev_[3], ev_[4]));
        }
        MXY_HIP(hipEventElapsedTime(&timing_.total_ms, ev_[0], ev_[4]));
        timing_.slices = ns;
    }
    if (last_.whole_lines && wl_) {   // the mode's counters came back behind the lookups; its intervals are the stream's
        const WholeLineCounters& h = *wl_->host.p;
        wl_->last[0] = h.queries; wl_->last[1] = h.address(); wl_->last[2] = h.string(); wl_->last[3] = h.invalid_utf8;
        out.n_cand = h.address() + h.string();   // the queries that were looked up
        if (profile_) { wl_->ms[0] = timing_.anchor_ms; wl_->ms[1] = timing_.validate_ms; wl_->ms[2] = timing_.lookup_ms; }
    }
}

// Queues the copies of what the caller asked for on `stream` (raw hits; final records from the mirror, or through the copy path with
// the optional sort; compact records; candidates) and points `out` at the pinned blocks. Returns the final records in the caller's
// order where they lie in device memory.
const FinalHit* Scanner::queue_record_copies(ScanOutput& out, bool want_cands, HitMode hit_mode, bool sorted, hipStream_t stream) {
    const ScanCounters& c = host_counters_;
    const int ns = n_slices_;
    out.hits.clear(); out.ids.clear(); out.cands.clear();
    out.fin = nullptr; out.fin_ids = nullptr; out.fin_offs = nullptr; out.n_fin = 0; out.n_fin_ids = 0;
    out.c4 = nullptr; out.n_c4 = 0;
    const bool had_mirror = mirror_used_;
    const FinalHit* dev_recs = final_.p;   // the records the caller gets, in its order, in device memory (line context)
    Work& w0 = work_[0];   // raw hits and candidate lists are read by one-slice scans only (single queries, extraction)
    const bool get_raw = last_.lookup && hit_mode == HITS_RAW && c.n_hits;
    const bool get_fin = last_.lookup && hit_mode == HITS_FINAL && c.n_final;
    if ((get_raw || want_cands) && ns != 1) throw HipError{"fetch: raw hits / candidates of a sliced scan"};
    // D2H into pinned memory (pageable destinations run at a fraction of the PCIe rate)
    if (get_raw) {
        ensure_pinned((size_t)c.n_hits * sizeof(Hit));
        MXY_HIP(hipMemcpyAsync(pinned_.p, w0.hits.p, (size_t)c.n_hits * sizeof(Hit), hipMemcpyDeviceToHost, stream));
        if (c.n_ids) {
            out.ids.resize(c.n_ids);
            MXY_HIP(hipMemcpyAsync(out.ids.data(), w0.ids.p, (size_t)c.n_ids * 4, hipMemcpyDeviceToHost, stream));
        }
    }
    if (get_fin && !sorted && mirror_used_ && c.n_final <= mirror_layout_.recs_cap && c.n_final_ids <= mirror_layout_.ids_cap) {
        // k_lookup (pack_record) has already written the records into pinned host memory
        const ResultArrays m = arrays_of(mirror_.p, mirror_layout_);
        out.fin = m.recs; out.n_fin = c.n_final;
        out.fin_ids = m.ids; out.fin_offs = m.offs; out.n_fin_ids = c.n_final_ids;
    } else if (get_fin) {
        if (mirror_used_ && !sorted) {  // did not fit: take the copy path now, have a larger mirror next time
            const uint32_t want_r = std::max((uint32_t)mirror_layout_.recs_cap, c.n_final + c.n_final / 2), want_i = std::max((uint32_t)mirror_layout_.ids_cap, c.n_final_ids + c.n_final_ids / 2);
            mirror_used_ = false;
            ensure_mirror(want_r, want_i);
        }
        const ResultLayout lay{c.n_final, c.n_final_ids};   // exactly the records of this scan
        ensure_pinned(lay.end());
        const ResultArrays h = arrays_of(pinned_.p, lay);
        const FinalHit* src = final_.p;
        if (sorted) {
            const uint32_t n = c.n_final;
            if (sort_keys_.n < 2 * (size_t)n) { sort_keys_.alloc(2 * (size_t)n + 2048); sort_vals_.alloc(2 * (size_t)n + 2048); final_sorted_.alloc((size_t)n + 1024); }
            const size_t tb = sort_hits_temp_bytes(n);
            if (sort_tmp_.n < tb) sort_tmp_.alloc(tb + tb / 4 + 4096);
            MXY_HIP(sort_hits(final_.p, n, sort_keys_.p, sort_vals_.p, sort_tmp_.p, tb, final_sorted_.p, stream));
            src = final_sorted_.p;
            dev_recs = src;
        }
        MXY_HIP(hipMemcpyAsync(h.recs, src, (size_t)c.n_final * sizeof(FinalHit), hipMemcpyDeviceToHost, stream));
        if (c.n_final_ids) {
            MXY_HIP(hipMemcpyAsync(h.ids, final_ids_.p, (size_t)c.n_final_ids * 4, hipMemcpyDeviceToHost, stream));
            MXY_HIP(hipMemcpyAsync(h.offs, final_offs_.p, (size_t)c.n_final_ids * 8, hipMemcpyDeviceToHost, stream));
        }
        out.fin = h.recs; out.n_fin = c.n_final;
        out.fin_ids = h.ids; out.fin_offs = h.offs; out.n_fin_ids = c.n_final_ids;
    }
    if (last_.lookup && hit_mode == HITS_FINAL && compact_ && c.n_c4) {
        if (had_mirror && !sorted && c.n_c4 <= mirror_c4_.n) out.c4 = mirror_c4_.p;   // written by the kernels
        else {
            if (had_mirror) { mirror_used_ = false; mirror_c4_.ensure(c.n_c4 + c.n_c4 / 2); }   // a larger mirror next time
            pinned_c4_.ensure(c.n_c4, c.n_c4 / 4 + 1024);
            MXY_HIP(hipMemcpyAsync(pinned_c4_.p, c4_.p, (size_t)c.n_c4 * sizeof(uint2), hipMemcpyDeviceToHost, stream));
            out.c4 = pinned_c4_.p;
        }
        out.n_c4 = c.n_c4;
    }
    const bool as_text = want_cands && extract_text_format_ >= 0 && !last_.lookup;   // the lists are rendered where they lie (queue_post_passes)
    if (want_cands && !unique_ && !as_text && c.n_cand + c.n_cand_a) {   // k_anchor's IPv4 list, then the validation kernels' list
        out.cands.resize((size_t)c.n_cand_a + c.n_cand);
        if (c.n_cand_a) MXY_HIP(hipMemcpyAsync(out.cands.data(), w0.cands_a.p, (size_t)c.n_cand_a * sizeof(Candidate), hipMemcpyDeviceToHost, stream));
        if (c.n_cand) MXY_HIP(hipMemcpyAsync(out.cands.data() + c.n_cand_a, w0.cands.p, (size_t)c.n_cand * sizeof(Candidate), hipMemcpyDeviceToHost, stream));
    }
    return dev_recs;
}

// The passes behind the scan, each over the records where they lie: line context, hit tally, segments (which reads the line context of
// this fetch), distinct texts.
void Scanner::queue_post_passes(ScanOutput& out, const FinalHit* dev_recs, bool want_cands, HitMode hit_mode, bool trace, hipStream_t stream) {
    const ScanCounters& c = host_counters_;
    Work& w0 = work_[0];
    const HitBatch batch{last_.ptr, last_.len, dev_recs, c.n_final, c4_.p, compact_ ? c.n_c4 : 0u};
    const bool to_host = hit_mode == HITS_FINAL;
    out.has_lines = false; out.fin_lines = nullptr; out.c4_lines = nullptr; out.lines_with_matches = 0;
    if (last_.lines && last_.lookup && !single_) {
        if (!lines_) lines_ = std::make_unique<LineContext>();
        lines_->resolve(batch, to_host, n_cu_, profile_, stream);
        out.has_lines = true;
    }
    // hit lines: the lines of the records, packed where the batch lies, behind the line records they are read from
    out.has_hit_lines = false; out.hit_lines = HitLinesView{};
    if (out.has_lines && last_.hit_lines) {
        if (!hit_lines_) hit_lines_ = std::make_unique<HitLines>();
        hit_lines_->resolve(batch, lines_->device_lines(), lines_->device_c4_lines(), c.lines, to_host, n_cu_, profile_, stream);
        out.has_hit_lines = true;
    }
    // hit tally: the records of the batch are counted where they lie, once per fetch — behind the regrow loop and the spill pass. With
    // set_profile or MATCHY_AMD_TRACE the pass times its kernels (one more host wait between them)
    if (tally_on_ && last_.lookup && !single_) {
        tally_->set_profile(profile_ || trace);
        tally_->add(last_.ptr, last_.len, final_.p, c.n_final, compact_ ? c4_.p : nullptr, compact_ ? c.n_c4 : 0u, stream);
        if (trace) {
            const HitTally::Events& ev = tally_->last_events();
            fprintf(stderr, "[matchy_amd] tally: %u records, %llu distinct (+%u), rehashes=%u pool_regrows=%u direct_adds=%u, claim %.3f ms publish %.3f ms total %.3f ms\n",
                    c.n_final + (compact_ ? c.n_c4 : 0u), (unsigned long long)tally_->distinct(), ev.new_entries, ev.rehashes, ev.pool_regrows, ev.direct_adds,
                    tally_->last_claim_ms(), tally_->last_publish_ms(), tally_->last_ms());
        }
    }
    // segmented scan: the records are attributed to the caller's segments where they lie, behind the line context it builds on
    out.has_segments = false; out.segments = nullptr; out.n_segments = 0; out.seg_of_fin = nullptr; out.seg_of_c4 = nullptr;
    if (segments_ && segments_->active() && last_.lookup && !single_) {
        const SegLines with_lines = out.has_lines ? SegLines{lines_->prefix(), lines_->set(), lines_->set_slots()} : SegLines{};
        segments_->resolve(batch, with_lines, to_host, profile_, stream);
        out.has_segments = true;
    }
    // rendered records: behind the line pass and the segment pass, whose device arrays it reads, over the records where they lie
    out.render = RenderView{};
    if (last_.render && render_ && last_.lookup && !single_) {
        RenderInput in;
        in.b = batch;
        in.data_offsets = reinterpret_cast<const int64_t*>(final_offs_.p); in.n_data_offsets = c.n_final_ids;
        if (out.has_lines) { in.fin_lines = lines_->device_lines(); in.c4_lines = lines_->device_c4_lines(); }
        if (out.has_segments) {
            in.n_segments = (uint32_t)segments_->armed_count();
            in.seg_of_fin = segments_->device_of_fin(); in.seg_of_c4 = segments_->device_of_c4();
            in.seg_line_base = out.has_lines ? segments_->device_line_base() : nullptr;
        }
        render_->resolve(in, to_host, n_cu_, profile_, stream);
        out.render.armed = true;
    }
    // candidates as text: both lists, or the first occurrences the handle's set leaves on the device, are ordered and written where they lie
    out.extract_text = ExtractTextView{};
    if (want_cands && extract_text_format_ >= 0 && !last_.lookup) {
        if (!extract_render_) extract_render_ = std::make_unique<ExtractRender>();
        XrInput in;
        in.data = last_.ptr; in.len = last_.len; in.format = (uint32_t)extract_text_format_;
        in.list_a = w0.cands_a.p; in.n_a = c.n_cand_a; in.list_b = w0.cands.p; in.n_b = c.n_cand; in.n_real = c.cand_true;
        if (last_.len > xrender::MAX_LEN || (uint64_t)c.n_cand_a + c.n_cand > 0xFFFFFFFFull) extract_render_->refuse();   // in front of the set: it stays as it is
        else {
            if (unique_) {
                in.n_real = distinct_->filter_device(last_.ptr, last_.len, w0.cands_a.p, c.n_cand_a, w0.cands.p, c.n_cand, c.cand_true, stream);
                in.list_a = distinct_->survivors(); in.n_a = in.n_real; in.list_b = nullptr; in.n_b = 0;
            }
            extract_render_->resolve(in, n_cu_, stream);
        }
        out.extract_text.armed = true;
    } else if (want_cands && unique_) {
        distinct_->filter(last_.ptr, last_.len, w0.cands_a.p, c.n_cand_a, w0.cands.p, c.n_cand, c.cand_true, out.cands, stream);
        if (trace) fprintf(stderr, "[matchy_amd] distinct: %zu of %u candidates are new, dedup %.3f ms behind %.3f ms of extraction kernels\n", out.cands.size(), c.cand_true,
                           distinct_->last_ms(), timing_.total_ms);
    }
}

// The wait for everything queued, what the passes read behind it, and the padding slots of partially filled chunks dropped.
void Scanner::finish_fetch(ScanOutput& out, bool want_cands, HitMode hit_mode, hipStream_t stream) {
    const ScanCounters& c = host_counters_;
    const bool get_raw = last_.lookup && hit_mode == HITS_RAW && c.n_hits;
    wait_stream(stream, last_.fork);
    if (out.has_lines) {
        const LineContext::Result r = lines_->finish();
        out.lines_with_matches = r.lines_with_matches; out.fin_lines = r.fin_lines; out.c4_lines = r.c4_lines;
    }
    if (out.has_hit_lines) {
        out.hit_lines = hit_lines_->finish();   // a second wait: the demand of the block is known only now
        if (getenv("MATCHY_AMD_TRACE") && !single_)
            fprintf(stderr, "[matchy_amd] hit lines: %u lines, block of %llu bytes, %llu bytes copied to the host\n", out.hit_lines.n_lines,
                    (unsigned long long)out.hit_lines.text_len, (unsigned long long)hit_lines_->last_copied_bytes());
    }
    if (out.has_segments) {
        const SegmentPass::Result r = segments_->finish();
        out.segments = r.segments; out.n_segments = r.n_segments; out.seg_of_fin = r.seg_of_fin; out.seg_of_c4 = r.seg_of_c4;
    }
    if (out.render.armed) {
        // further waits: payloads the table missed are rendered here and the pass repeated; the demand of the block is known only now
        out.render = render_->finish(&payload_json, img_.get());
        if (getenv("MATCHY_AMD_TRACE") && !single_) {
            const NdjsonRender::Events& ev = render_->last_events();
            fprintf(stderr, "[matchy_amd] render: block of %llu bytes, status %u, %u repeats, %llu misses, %u payloads rendered, %llu bytes copied to the host\n",
                    (unsigned long long)out.render.len, out.render.status, ev.rounds, (unsigned long long)ev.misses, ev.payloads_added, (unsigned long long)ev.copied);
        }
    }
    // drop the padding slots of partially filled chunks
    if (get_raw) {
        const Hit* ph = (const Hit*)pinned_.p;
        out.hits.reserve(c.hits_true);
        for (size_t r = 0; r < c.n_hits; ++r) if (ph[r].kind != 0xFF) out.hits.push_back(ph[r]);
    }
    if (!out.cands.empty()) {
        size_t w = 0;
        for (size_t r = 0; r < out.cands.size(); ++r) if (out.cands[r].len_type != 0xFFFFFFFFu) out.cands[w++] = out.cands[r];
        out.cands.resize(w);
    }
    for (auto& t : out.by_type) t = 0;
    if (want_cands) for (const Candidate& cd : out.cands) { uint32_t ty = cd.len_type >> 24; if (ty < IT_COUNT) out.by_type[ty]++; }
    if (out.extract_text.armed) {
        out.extract_text = extract_render_->finish();   // a second wait: the demand of the block is known only now
        for (int t = 0; t < IT_COUNT; ++t) out.by_type[t] = out.extract_text.by_type[t];
        if (getenv("MATCHY_AMD_TRACE")) {
            float ms[4];
            extract_render_->timing(ms);
            fprintf(stderr, "[matchy_amd] extract text: %llu records, block of %llu bytes, status %u; keys + sort %.3f ms, measure %.3f ms, write %.3f ms, copy %.3f ms, behind %.3f ms of extraction kernels\n",
                    (unsigned long long)out.extract_text.n_records, (unsigned long long)out.extract_text.len, out.extract_text.status, ms[0], ms[1], ms[2], ms[3],
                    timing_.total_ms);
        }
    }
}

void Scanner::fetch(ScanOutput& out, bool want_cands, hipStream_t stream, HitMode hit_mode, bool sorted) {
    const bool trace = !single_ && getenv("MATCHY_AMD_TRACE");
    MXY_HIP(hipSetDevice(ddb_->device));   // regrown buffers must land on this scanner's device whatever thread calls
    const auto t_begin = std::chrono::steady_clock::now();
    auto since = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count(); };
    settle_counters(trace, stream);
    const double t_counters = since();
    report_counters(out, trace);
    const FinalHit* dev_recs = queue_record_copies(out, want_cands, hit_mode, sorted, stream);
    queue_post_passes(out, dev_recs, want_cands, hit_mode, trace, stream);
    finish_fetch(out, want_cands, hit_mode, stream);
    if (trace) fprintf(stderr, "[matchy_amd] fetch: counters after %.3f ms, records after %.3f ms\n", t_counters, since());
}

// Rendered records (render.h). The parameters are the caller's until arm_render() takes them for one scan.
void payload_json(const void* img, uint32_t data_off, std::string& json) {
    json.clear();
    DataValue dv;
    if (static_cast<const DbImage*>(img)->decode_data(data_off, dv)) to_json(dv, json); else json = "null";
}

void Scanner::set_render(const RenderParams* p) {
    render_pending_.reset(p ? new RenderParams(*p) : nullptr);
}

void Scanner::arm_render(ScanRequest& rq, bool fetch_renders, hipStream_t stream) {
    rq.render = false;
    if (!render_pending_) return;
    const std::unique_ptr<RenderParams> p = std::move(render_pending_);
    if (!fetch_renders || !rq.lookup) return;
    if ((p->flags & (render::FLAG_LINE_NUMBERS | render::FLAG_INPUT_LINE)) && !rq.lines)
        throw ParamError{"set_render: line numbers and input lines need line context (set_line_context)"};
    const size_t n_segments = segments_ ? segments_->armed_count() : 0;
    if (p->per_segment && !n_segments) throw ParamError{"set_render: sources are given per segment, and the scan has no segments"};
    if (p->per_segment && p->sources.size() != n_segments)
        throw ParamError{"set_render: " + std::to_string(p->sources.size()) + " sources for a scan of " + std::to_string(n_segments) + " segments"};
    MXY_HIP(hipSetDevice(ddb_->device));
    if (!render_) render_ = std::make_unique<NdjsonRender>();
    render_->arm(*p, stream);
    rq.render = true;
}

// Segmented scans (segments.h). The table is the caller's until arm_segments() takes it for one scan.
void Scanner::set_segments(const uint32_t* starts, size_t n) {
    if (!segments_ && starts && n) segments_ = std::make_unique<SegmentPass>();
    if (segments_) segments_->set(starts, n);
}

void Scanner::arm_segments(size_t len, hipStream_t stream, bool upload) {
    if (!segments_) return;
    segments_->arm(len);
    if (!segments_->active() || !upload) return;
    MXY_HIP(hipSetDevice(ddb_->device));
    segments_->upload(stream);
}

// gz scans (inflate.h). The pass and the scan behind it share this scanner's own stream, so nothing waits on the host in between.
template <class Launch>
Scanner::GzBatch Scanner::gz_pass(Launch&& launch) {
    MXY_HIP(hipSetDevice(ddb_->device));
    host_stream_.create(hipStreamNonBlocking);
    if (!gz_) gz_ = std::make_unique<GzInflate>();
    gz_->set_pieces(gz_piece_bytes_);
    launch(*gz_);
    set_segments(gz_->starts().data(), gz_->starts().size());
    return GzBatch{gz_->device_text(), gz_->text_len(), host_stream_};
}
Scanner::GzBatch Scanner::gz_inflate(const uint8_t* packed, size_t packed_len, const GzMemberIn* members, size_t n) {
    return gz_pass([&](GzInflate& g) { g.launch(packed, packed_len, members, n, n_cu_, profile_, host_stream_); });
}
Scanner::GzBatch Scanner::gz_inflate_files(const uint8_t* packed, size_t packed_len, const GzFileIn* files, size_t n_files) {
    return gz_pass([&](GzInflate& g) { g.launch_files(packed, packed_len, files, n_files, n_cu_, profile_, host_stream_); });
}
Scanner::GzBatch Scanner::gz_inflate_window(const uint8_t* packed, size_t packed_len, const uint8_t* carry, uint32_t carry_len, uint32_t carry_cap, bool last) {
    return gz_pass([&](GzInflate& g) { g.launch_window(packed, packed_len, carry, carry_len, carry_cap, last, n_cu_, profile_, host_stream_); });
}
Scanner::GzBatch Scanner::gz_inflate_stream(const uint8_t* packed, size_t packed_len, const gz::StreamState* state, const uint8_t* carry, uint32_t carry_len, uint32_t carry_cap,
                                            uint32_t text_cap, bool first, bool file_end) {
    return gz_pass([&](GzInflate& g) { g.launch_stream(packed, packed_len, state, carry, carry_len, carry_cap, text_cap, first, file_end, n_cu_, profile_, host_stream_); });
}
void Scanner::gz_queue_results(bool want_text) { gz_->queue_results(want_text, host_stream_); }
GzInflate::Result Scanner::gz_finish() { return gz_->finish(); }

// The input of a front pass (utf16.h, unescape.h): device memory is read where it lies when it is aligned for 16-byte loads; device
// memory that is not is copied, and host memory travels the way a piece of scan_host does — the whole pages inside it pinned for the
// copy (or found pinned by this library), the bytes in front of and behind them as they are
template <class Pass>
const uint8_t* Scanner::front_pass_input(Pass& pass, HostPin& pin, const uint8_t* src, size_t len) {
    pin.release();
    hipPointerAttribute_t attr{};
    const bool on_device = len && hipPointerGetAttributes(&attr, src) == hipSuccess && attr.type == hipMemoryTypeDevice;
    if (len && !on_device) (void)hipGetLastError();   // a plain host pointer is no error
    if (on_device && ((uintptr_t)src & 15u)) {
        uint8_t* dst = pass.input_buffer(len);
        MXY_HIP(hipMemcpyAsync(dst, src, len, hipMemcpyDeviceToDevice, host_stream_));
        return dst;
    }
    if (len && !on_device) {
        uint8_t* dst = pass.input_buffer(len);
        static const bool no_reg = getenv("MATCHY_AMD_NO_REGISTER") != nullptr;
        uintptr_t a = 0, b = 0;
        if (!no_reg && len >= ((size_t)4 << 20) && inner_pages(src, len, a, b) && pins::acquire(a, b)) {
            pin.a = a; pin.b = b;
            const size_t head = (size_t)(a - (uintptr_t)src), mid = (size_t)(b - a), tail = len - head - mid;
            if (head) MXY_HIP(hipMemcpyAsync(dst, src, head, hipMemcpyHostToDevice, host_stream_));
            MXY_HIP(hipMemcpyAsync(dst + head, (const void*)a, mid, hipMemcpyHostToDevice, host_stream_));
            if (tail) MXY_HIP(hipMemcpyAsync(dst + head + mid, (const void*)b, tail, hipMemcpyHostToDevice, host_stream_));
        } else MXY_HIP(hipMemcpyAsync(dst, src, len, hipMemcpyHostToDevice, host_stream_));
        return dst;
    }
    return src;
}

// UTF-16 inputs (utf16.h). Like a gz scan, the pass and the scan behind it share this scanner's own stream.
Scanner::GzBatch Scanner::utf16_transcode(const uint8_t* src, size_t len, uint32_t byte_order) {
    if (segments_ && segments_->pending()) {
        set_segments(nullptr, 0);
        throw ParamError{"UTF-16 inputs and segments cannot be combined"};
    }
    if (whole_lines_) throw ParamError{"UTF-16 inputs and whole-line mode cannot be combined"};
    Utf16Transcode::check(src, len, byte_order);
    MXY_HIP(hipSetDevice(ddb_->device));
    host_stream_.create(hipStreamNonBlocking);
    if (!utf16_) utf16_ = std::make_unique<Utf16Transcode>();
    const uint8_t* in = front_pass_input(*utf16_, utf16_pin_, src, len);
    utf16_->launch(in, len, byte_order, n_cu_, true, host_stream_);   // always timed: four event records per batch, for `matchy match -s`
    return GzBatch{utf16_->device_text(), utf16_->text_len(), host_stream_};
}
void Scanner::HostPin::release() { if (b > a) pins::release(a, b); a = b = 0; }
void Scanner::utf16_queue_text(bool want_text) { utf16_->queue_results(want_text, host_stream_); }
Utf16Transcode::Result Scanner::utf16_finish() {
    const Utf16Transcode::Result r = utf16_->finish();
    utf16_pin_.release();   // behind the fetch: the copy is done
    return r;
}

// Percent- and JSON-escaped inputs (unescape.h): the same shape
Scanner::GzBatch Scanner::unescape(const uint8_t* src, size_t len, uint32_t modes) {
    if (segments_ && segments_->pending()) {
        set_segments(nullptr, 0);
        throw ParamError{"escaped inputs and segments cannot be combined"};
    }
    if (whole_lines_) throw ParamError{"escaped inputs and whole-line mode cannot be combined"};
    Unescape::check(src, len, modes);
    MXY_HIP(hipSetDevice(ddb_->device));
    host_stream_.create(hipStreamNonBlocking);
    if (!unescape_) unescape_ = std::make_unique<Unescape>();
    const uint8_t* in = front_pass_input(*unescape_, unescape_pin_, src, len);
    unescape_->launch(in, len, modes, n_cu_, true, host_stream_);   // always timed, like the UTF-16 pass
    return GzBatch{unescape_->device_text(), unescape_->text_len(), host_stream_};
}
void Scanner::unescape_queue_text(bool want_text) { unescape_->queue_results(want_text, host_stream_); }
Unescape::Result Scanner::unescape_finish() {
    const Unescape::Result r = unescape_->finish();
    unescape_pin_.release();   // behind the fetch: the copy is done
    return r;
}

size_t host_piece_bytes() {
    static const size_t v = [] {
        const unsigned long long maxc = 1ull << 30;
        const char* e = getenv("MATCHY_AMD_HOST_PIECE_BYTES");
        if (!e || !*e) return (size_t)maxc;
        return (size_t)std::min(std::max(strtoull(e, nullptr, 10), 1ull), maxc);
    }();
    return v;
}

// Spill pass of the glob lookup (k_lookup_spill): list of candidate indices per slice; the per-thread scratch (one bit per
// pattern id and a star stack as deep as the longest pattern: ~128 MB for a million patterns) is allocated by fetch() when a
// scan has actually spilled.
void Scanner::setup_spill(int sl, LookupParams& lp) {
    if (!ddb_->view.has_glob) return;
    Work& w = work_[sl];
    const size_t words = (ddb_->view.pattern_count + 31) / 32 + 2 * ((size_t)ddb_->view.glob_max_segs + 1);
    const size_t want = std::max<size_t>(1024, w.cands.n / 256);
    if (w.spill.n < want) w.spill.alloc(want);
    lp.spill = w.spill.p; lp.spill_cap = (uint32_t)w.spill.n;
    lp.spill_scratch = nullptr; lp.spill_words = (uint32_t)words; lp.spill_blocks = SPILL_BLOCKS;
}

void Scanner::lookup_one(const std::string& text, Candidate c, ScanOutput& out) {
    MXY_HIP(hipSetDevice(ddb_->device));
    ensure_capacity(4096);
    Work& w = work_[0];
    if (staging_.n < text.size() + 16) staging_.alloc(text.size() + 4096);
    if (!text.empty()) MXY_HIP(hipMemcpy(staging_.p, text.data(), text.size(), hipMemcpyHostToDevice));
    c.start = 0;
    MXY_HIP(hipMemcpy(w.cands.p, &c, sizeof(c), hipMemcpyHostToDevice));
    ScanCounters z{};
    z.n_cand = 1;
    MXY_HIP(hipMemcpy(counters_.p, &z, sizeof(z), hipMemcpyHostToDevice));
    counters_clean_ = false;
    LookupParams lp{};
    lp.log = staging_.p; lp.len = (uint32_t)text.size(); lp.cands = w.cands.p; lp.cand_cap = (uint32_t)w.cands.n;
    lp.hits = w.hits.p; lp.hit_cap = (uint32_t)w.hits.n; lp.ids = w.ids.p; lp.ids_cap = (uint32_t)w.ids.n;
    lp.counters = counters_.p;
    setup_spill(0, lp);
    launch_lookup(lp, ddb_->view, 1, nullptr);
    launch_[0].lp = lp;   // fetch() launches the spill pass from here if the candidate spilled
    n_slices_ = 1; spill_done_ = false;
    last_.lookup = true; last_.ptr = staging_.p; last_.len = (uint32_t)text.size();
    // a single query is fetched untimed and as raw hits; both switches go back however fetch() ends
    struct Single {
        Scanner& s; const bool prof;
        explicit Single(Scanner& sc) : s(sc), prof(sc.profile_) { s.profile_ = false; s.single_ = true; }
        ~Single() { s.single_ = false; s.profile_ = prof; }
    } single(*this);
    fetch(out, false, nullptr, HITS_RAW);
}

void Scanner::scan_host(const uint8_t* data, size_t len, bool lookup, bool want_cands, ScanOutput& out, std::vector<uint64_t>* cand_bases,
                        std::vector<FinalHit>* fin, std::vector<uint32_t>* fin_ids, std::vector<long long>* fin_offs, std::vector<LineRec>* fin_lines) {
    // Cut into < 2^30-byte pieces at newlines (N4 in SURVEY §8a: no candidate class admits '\n').
    const size_t MAXC = host_piece_bytes();
    // the calling thread may be another one than last time (its current device is thread state): allocations below must land
    // on this scanner's device
    MXY_HIP(hipSetDevice(ddb_->device));
    // copies and kernels of a host-buffer scan go to a stream of this scanner's own, so that several scanners on one
    // device (one per host thread, `matchy match --devices 0,0`) overlap one batch's transfer with another's kernels
    host_stream_.create(hipStreamNonBlocking);
    out = ScanOutput();
    size_t pos = 0;
    std::vector<Candidate> all_cands;
    if (cand_bases) cand_bases->clear();
    if (fin) { fin->clear(); fin_ids->clear(); fin_offs->clear(); }
    if (fin_lines) fin_lines->clear();
    // whole-line mode: the pieces are cut at newlines, which is the cut the mode needs; its counters add up over them
    ScanRequest mode;
    mode.lookup = lookup;
    arm_whole_lines(mode);
    uint64_t wl_sum[4] = {0, 0, 0, 0};
    // segmented scan: every piece gets the starts that intersect it, clamped and shifted; a piece ends at a line end, so the per-segment
    // figures of the pieces add up, and the indices go back into the caller's table
    std::vector<uint32_t> seg_all;
    if (lookup && segments_) {
        arm_segments(len, host_stream_, false);   // the whole table; every piece uploads its own below
        seg_all = segments_->take();
    }
    const SegmentPass::OffAtExit seg_off{segments_.get()};
    if (!seg_all.empty()) {
        out.seg_own.resize(seg_all.size());
        for (size_t s = 0; s < seg_all.size(); ++s) {
            SegmentRec r{};
            r.start = seg_all[s];
            r.len = (s + 1 < seg_all.size() ? seg_all[s + 1] : (uint32_t)len) - seg_all[s];
            out.seg_own[s] = r;
        }
    }
    // rendered records: the parameters of set_render arm every piece, with the lines of the pieces in front added to the line bases
    const std::unique_ptr<RenderParams> render_all = std::move(render_pending_);
    const bool render_on = render_all && lookup && fin;
    if (render_on) {
        if ((render_all->flags & (render::FLAG_LINE_NUMBERS | render::FLAG_INPUT_LINE)) && !(line_ctx_ || hit_lines_on_))
            throw ParamError{"set_render: line numbers and input lines need line context (set_line_context)"};
        if (render_all->per_segment && seg_all.empty()) throw ParamError{"set_render: sources are given per segment, and the scan has no segments"};
        if (render_all->per_segment && render_all->sources.size() != seg_all.size())
            throw ParamError{"set_render: " + std::to_string(render_all->sources.size()) + " sources for a scan of " + std::to_string(seg_all.size()) + " segments"};
        out.render = RenderView{};
        out.render.armed = true;
        out.render_own.clear();
    }
    // candidates as text: the blocks of the pieces go end to end into one pinned block, the counts add up
    const bool as_text = want_cands && extract_text_format_ >= 0 && !lookup;
    if (as_text) {
        if (!extract_render_) extract_render_ = std::make_unique<ExtractRender>();
        extract_render_->begin();
        out.extract_text.armed = true;
    }
    do {
        const size_t n = newline_cut(data, pos, len, MAXC) - pos;
        if (n > ((size_t)1 << 30)) throw HipError{"scan_host: a single line exceeds 1 GiB"};
        if (staging_.n < n + 16) staging_.alloc(n + 16 + n / 8);
        // Pageable host memory (a mapped file, a heap buffer) reaches the device through the runtime's own pinned staging at
        // ~20 GB/s; pinned for the duration of the copy (hipHostRegister: ~5 ms per GB, tools/ubench/h2d_rate2.cpp) the DMA
        // engine reads the pages themselves at the bus rate (~57 GB/s). Only whole pages inside the piece are registered —
        // neighbouring pieces (other scanners working on the same mapping) never share a page of their registered ranges —
        // the few bytes in front of and behind them travel as they did. Memory that is pinned already, small pieces and
        // MATCHY_AMD_NO_REGISTER=1 take the plain copy.
        const bool trace_h = getenv("MATCHY_AMD_TRACE") != nullptr;
        const auto th0 = std::chrono::steady_clock::now();
        auto ms_since = [&](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); };
        const uint8_t* src = data + pos;
        const uint8_t* reg_lo = nullptr;
        size_t reg_len = 0;
        bool mine = false;   // this call pinned the range (and unpins it)
        static const bool no_reg = getenv("MATCHY_AMD_NO_REGISTER") != nullptr;
        if (!no_reg && n >= ((size_t)4 << 20)) {
            uintptr_t a, b;
            // pins::acquire: the whole range is covered by a pin of this library (the caller's, or another scanner's transient one —
            // its count goes up, so it stays pinned until this copy is done too), or it is pinned now. Anything else (memory someone
            // else pinned, a partial overlap, a failed registration) takes the one plain copy below.
            if (inner_pages(src, n, a, b) && pins::acquire(a, b)) { reg_lo = (const uint8_t*)a; reg_len = b - a; mine = true; }
        }
        struct Unreg { uintptr_t a, b; ~Unreg() { if (b > a) pins::release(a, b); } } unreg{mine ? (uintptr_t)reg_lo : 0, mine ? (uintptr_t)reg_lo + reg_len : 0};
        const double t_reg = ms_since(th0);
        if (reg_lo) {
            const size_t head = (size_t)(reg_lo - src), tail = n - head - reg_len;
            if (head) MXY_HIP(hipMemcpyAsync(staging_.p, src, head, hipMemcpyHostToDevice, host_stream_));
            MXY_HIP(hipMemcpyAsync(staging_.p + head, reg_lo, reg_len, hipMemcpyHostToDevice, host_stream_));
            if (tail) MXY_HIP(hipMemcpyAsync(staging_.p + head + reg_len, reg_lo + reg_len, tail, hipMemcpyHostToDevice, host_stream_));
        } else if (n) MXY_HIP(hipMemcpyAsync(staging_.p, src, n, hipMemcpyHostToDevice, host_stream_));
        ScanRequest rq;
        rq.ptr = staging_.p; rq.len = (uint32_t)n; rq.lookup = lookup; rq.lines = (line_ctx_ || hit_lines_on_) && lookup;
        rq.hit_lines = hit_lines_on_ && lookup && fin;
        rq.whole_lines = mode.whole_lines;
        size_t seg_first = 0, seg_last = 0;
        if (!seg_all.empty()) {
            // the last segment that starts at or in front of the piece .. the last that starts inside it (the last piece: the last of all)
            // (a run of empty segments that starts exactly at the piece's start belongs to this piece: from the first start equal to pos)
            const size_t at_pos = (size_t)(std::lower_bound(seg_all.begin(), seg_all.end(), (uint32_t)pos) - seg_all.begin());
            seg_first = at_pos < seg_all.size() && seg_all[at_pos] == pos ? at_pos : at_pos - 1;
            seg_last = pos + n >= len ? seg_all.size() - 1 : (size_t)(std::lower_bound(seg_all.begin(), seg_all.end(), (uint32_t)(pos + n)) - seg_all.begin()) - 1;
            segments_->arm_piece(seg_all, seg_first, seg_last, (uint32_t)pos);
            segments_->upload(host_stream_);
        }
        if (render_on) {
            // a segment that began in an earlier piece goes on at the piece's first byte: its lines so far join its base
            RenderParams p;
            p.flags = render_all->flags; p.per_segment = render_all->per_segment;
            if (p.per_segment)
                for (size_t k = seg_first; k <= seg_last; ++k) { p.sources.push_back(render_all->sources[k]); p.line_bases.push_back(render_all->line_bases[k] + out.seg_own[k].lines); }
            else { p.sources = render_all->sources; p.line_bases.assign(1, (render_all->line_bases.empty() ? 0 : render_all->line_bases[0]) + out.lines); }
            if (!render_) render_ = std::make_unique<NdjsonRender>();
            render_->arm(p, host_stream_);
            rq.render = true;
        }
        scan_device(rq, host_stream_);
        ScanOutput part;
        const double t_launch = ms_since(th0);
        fetch(part, want_cands, host_stream_, lookup && fin ? HITS_FINAL : HITS_NONE, true);   // synchronises the stream: the copy is done
        if (trace_h) {
            static const auto t_proc = std::chrono::steady_clock::now();
            fprintf(stderr, "[matchy_amd] t=%.1f ms scan_host piece %zu B: registered %zu B in %.3f ms, launches done after %.3f ms, results after %.3f ms\n",
                    ms_since(t_proc), n, reg_len, t_reg, t_launch, ms_since(th0));
        }
        // a line never spans a cut: the pieces' distinct lines add up, and a piece's line numbers continue the count of the earlier pieces
        if (part.has_lines) {
            out.has_lines = true; out.lines_with_matches += part.lines_with_matches;
            if (fin_lines && part.n_fin) append_shifted_lines(part.fin_lines, part.n_fin, (uint32_t)pos, (uint32_t)out.lines, *fin_lines);
        }
        // a piece renders its own records: the blocks go end to end, and one piece that was too large is the verdict of the whole
        if (part.render.armed) {
            if (part.render.status != RENDER_OK) out.render.status = part.render.status;
            else if (part.render.len) out.render_own.insert(out.render_own.end(), part.render.text, part.render.text + part.render.len);
        }
        if (part.extract_text.armed) {
            ExtractTextView& v = out.extract_text;
            if (part.extract_text.status != XR_OK) v.status = part.extract_text.status;
            v.n_records += part.extract_text.n_records;
            for (int t = 0; t < IT_COUNT; ++t) v.by_type[t] += part.extract_text.by_type[t];
        }
        // a piece ends at a line end: its block goes behind the blocks of the pieces in front of it
        if (part.has_hit_lines) {
            out.has_hit_lines = true;
            const HitLinesView& v = part.hit_lines;
            const uint32_t text_base = (uint32_t)out.hl_text_own.size(), k_base = (uint32_t)out.hl_no_own.size();
            if (out.hl_off_own.empty()) out.hl_off_own.push_back(0);
            for (uint32_t k = 0; k < v.n_lines; ++k) { out.hl_off_own.push_back(text_base + v.line_off[k + 1]); out.hl_no_own.push_back((uint32_t)out.lines + v.line_no[k]); }
            for (size_t i = 0; i < part.n_fin; ++i) out.hl_of_own.push_back(k_base + v.line_of_fin[i]);
            if ((uint64_t)text_base + v.text_len > 0xFFFFFFFFull) throw HipError{"scan_host: the hit lines of the pieces exceed 4 GiB (32-bit offsets)"};
            if (v.text_len) out.hl_text_own.insert(out.hl_text_own.end(), v.text, v.text + v.text_len);
        }
        if (part.has_segments) {
            out.has_segments = true;
            for (size_t k = 0; k < part.n_segments; ++k) {
                SegmentRec& g = out.seg_own[seg_first + k];
                const SegmentRec& p = part.segments[k];
                g.hits += p.hits; g.lines += p.lines; g.lines_with_matches += p.lines_with_matches;
                if (part.has_lines && seg_all[seg_first + k] >= pos) g.line_base = (uint32_t)out.lines + p.line_base;   // the segment starts in this piece
            }
            if (part.seg_of_fin) for (size_t i = 0; i < part.n_fin; ++i) out.seg_of_own.push_back(part.seg_of_fin[i] + (uint32_t)seg_first);
        }
        out.lines += part.lines; out.n_cand += part.n_cand; out.n_hits += part.n_hits;
        if (mode.whole_lines) for (int k = 0; k < 4; ++k) wl_sum[k] += wl_->last[k];
        for (int t = 0; t < IT_COUNT; ++t) out.by_type[t] += part.by_type[t];
        if (fin && part.n_fin) append_shifted(part.fin, part.n_fin, part.fin_ids, part.fin_offs, part.n_fin_ids, (uint32_t)pos, *fin, *fin_ids, *fin_offs);
        for (const Candidate& c : part.cands) { all_cands.push_back(c); if (cand_bases) cand_bases->push_back(pos); }
        pos += n;
    } while (pos < len);
    out.cands.swap(all_cands);
    if (mode.whole_lines) for (int k = 0; k < 4; ++k) wl_->last[k] = wl_sum[k];
    if (out.has_hit_lines) {
        HitLinesView& v = out.hit_lines;
        v.text = out.hl_text_own.empty() ? nullptr : out.hl_text_own.data(); v.text_len = out.hl_text_own.size();
        v.n_lines = (uint32_t)out.hl_no_own.size();
        v.line_off = out.hl_off_own.data(); v.line_no = out.hl_no_own.empty() ? nullptr : out.hl_no_own.data();
        v.line_of_fin = out.hl_of_own.empty() ? nullptr : out.hl_of_own.data(); v.line_of_c4 = nullptr;
    }
    if (as_text && out.extract_text.status == XR_OK) { out.extract_text.text = extract_render_->joined(); out.extract_text.len = extract_render_->joined_len(); }
    if (out.render.armed && out.render.status == RENDER_OK) { out.render.text = out.render_own.empty() ? nullptr : out.render_own.data(); out.render.len = out.render_own.size(); }
    if (out.has_segments) {
        out.segments = out.seg_own.data(); out.n_segments = out.seg_own.size();
        out.seg_of_fin = out.seg_of_own.empty() ? nullptr : out.seg_of_own.data();
    }
}

namespace pins {
namespace {
struct Entry { uintptr_t a, b; int refs; bool caller; };
std::mutex g_mutex;
std::vector<Entry> g_entries;
}  // namespace
bool acquire(uintptr_t a, uintptr_t b) {
    std::lock_guard<std::mutex> lock(g_mutex);
    for (Entry& e : g_entries) {
        if (e.a <= a && b <= e.b) { ++e.refs; return true; }
        if (a < e.b && e.a < b) return false;   // partial overlap with a pinned range: registering would fail, a pinned-path copy would run over unpinned pages
    }
    const hipError_t err = hipHostRegister((void*)a, b - a, hipHostRegisterDefault);
    if (err != hipSuccess) { (void)hipGetLastError(); return false; }   // pinned by someone else (hipHostMalloc, a foreign registration) or not pinnable
    g_entries.push_back(Entry{a, b, 1, false});
    return true;
}
void release(uintptr_t a, uintptr_t b) {
    std::lock_guard<std::mutex> lock(g_mutex);
    for (size_t i = 0; i < g_entries.size(); ++i) {
        Entry& e = g_entries[i];
        if (!(e.a <= a && b <= e.b) || e.refs <= 0) continue;
        if (--e.refs == 0 && !e.caller) {
            (void)hipHostUnregister((void*)e.a);
            (void)hipGetLastError();
            g_entries.erase(g_entries.begin() + (long)i);
        }
        return;
    }
}
int add_caller(const void* ptr, size_t bytes) {
    std::lock_guard<std::mutex> lock(g_mutex);
    if (hipHostRegister(const_cast<void*>(ptr), bytes, hipHostRegisterDefault) != hipSuccess) { (void)hipGetLastError(); return -1; }
    g_entries.push_back(Entry{(uintptr_t)ptr, (uintptr_t)ptr + bytes, 1, true});   // the caller's own reference
    return 0;
}
void remove_caller(const void* ptr) {
    std::lock_guard<std::mutex> lock(g_mutex);
    for (size_t i = 0; i < g_entries.size(); ++i) {
        if (g_entries[i].a != (uintptr_t)ptr || !g_entries[i].caller) continue;
        // the caller says the range is no longer in use (it must not unregister under its own scans): drop it whatever the count
        (void)hipHostUnregister(const_cast<void*>(ptr));
        (void)hipGetLastError();
        g_entries.erase(g_entries.begin() + (long)i);
        return;
    }
    (void)hipHostUnregister(const_cast<void*>(ptr));   // not registered through this library: as before
    (void)hipGetLastError();
}
}  // namespace pins

}  // namespace mxy
