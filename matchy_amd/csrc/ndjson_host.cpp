#include "ndjson_host.h"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <thread>
#include <vector>

#include "data_codec.h"
#include "render_core.h"
#include "utf8_lossy.h"

namespace mxy {
namespace ndjson {
namespace {

// The sink of render::record_emit that appends to a std::string. Both escaped fields go by the per-byte rules of render_core.h, a run
// of bytes that stand for themselves in one append (extracted items are almost always plain ASCII without '"' or a backslash).
struct StringSink {
    std::string& o;
    std::string& lossy;   // scratch of line()
    void lit(const char* p, uint32_t len) { o.append(p, len); }
    void bytes(const uint8_t* p, uint32_t len) { o.append(reinterpret_cast<const char*>(p), len); }
    void text(const uint8_t* f, size_t len) {
        for (size_t i = 0; i < len;) {
            size_t j = i;
            while (j < len && render::esc_len(f[j]) == 1) ++j;
            o.append(reinterpret_cast<const char*>(f) + i, j - i);
            if (j < len) { uint8_t t[render::BYTE_TEXT_MAX]; o.append(reinterpret_cast<const char*>(t), render::esc_put(f[j++], t)); }
            i = j;
        }
    }
    void text_inline(const uint8_t* f, uint32_t len) { text(f, len); }
    void line(const uint8_t* f, uint32_t len) {
        if (std::all_of(f, f + len, [](uint8_t c) { return c < 0x80; })) return text(f, len);   // utf8_lossy leaves ASCII alone
        lossy.clear();
        utf8_lossy_append(f, len, lossy);
        text(reinterpret_cast<const uint8_t*>(lossy.data()), lossy.size());
    }
    void dec(uint64_t v) { uint8_t t[20]; o.append(reinterpret_cast<const char*>(t), render::dec_put(v, t)); }
};

// One piece of a result: its text and the payloads it rendered itself (the strings of an unordered_map stay where they are).
struct Piece { std::string o; std::unordered_map<uint32_t, std::string> fresh; };

// The payload texts of record_emit. While pieces are rendered the cache is only read, by several threads at once: a payload that is not
// in it yet is rendered into the piece's own map and joins the cache behind the threads.
struct PayloadTexts {
    const std::unordered_map<uint32_t, std::string>* cache;   // NULL: none
    Piece& pc;
    Payloads pay;
    const int64_t* data_offsets;
    const std::string& json(uint32_t off) {
        if (cache) { const auto it = cache->find(off); if (it != cache->end()) return it->second; }
        const auto ins = pc.fresh.emplace(off, std::string());
        if (ins.second) pay.fn(pay.ctx, off, ins.first->second);
        return ins.first->second;
    }
    template <class S> void one(S& s, uint32_t off) {
        const std::string& j = json(off);
        s.bytes(reinterpret_cast<const uint8_t*>(j.data()), (uint32_t)j.size());
    }
    template <class S> void array(S& s, uint32_t first, uint32_t n) {
        bool any = false;
        for (uint32_t k = 0; k < n; ++k) {
            const int64_t off = data_offsets[first + k];
            if (off < 0) continue;
            if (any) MXY_RC_LIT(s, ","); else MXY_RC_LIT(s, "\"data\":[");
            one(s, (uint32_t)off);
            any = true;
        }
        if (any) MXY_RC_LIT(s, "],");
    }
};

// The text of record i and its whole line inside the block of hit lines; false when the block does not have them.
struct BlockLine { const uint8_t* hit; const uint8_t* line; uint32_t line_len; };
bool block_line_of(const ResultView& v, bool in_hits, size_t i, uint32_t hit_start, BlockLine& bl) {
    if (!v.block || !v.block->text) return false;
    const matchy_scan_hit_lines_t& h = *v.block;
    const uint32_t* of = in_hits ? h.line_of_hit : h.line_of_ip4_hit;
    const matchy_scan_line_t* ln = in_hits ? v.lines : v.ip4_lines;
    if (!of || !ln) return false;
    const uint32_t k = of[i];
    if (k >= h.n_lines) return false;
    bl.line = h.text + h.line_off[k];
    bl.line_len = h.line_off[k + 1] - 1u - h.line_off[k];
    bl.hit = bl.line + (hit_start - ln[i].line_start);
    return true;
}

std::string escaped(const char* source) { std::string o; json_escape(source ? source : "-", o); return o; }

struct Joiner { std::vector<std::thread>& t; ~Joiner() { for (auto& x : t) if (x.joinable()) x.join(); } };

}  // namespace

bool Renderer::record(const ResultView& v, bool in_hits, size_t i, const char* source, Payloads pay, std::string& out) {
    const matchy_scan_hit_t h = in_hits ? v.hits[i] : matchy_scan_ip4_hit_expand(v.ip4_hits[i]);
    BlockLine bl{};
    const bool from_block = block_line_of(v, in_hits, i, h.start, bl);
    if (!from_block && !v.text) return false;
    const std::string src = escaped(source);
    render::RecordIn r{from_block ? bl.hit : v.text + h.start, MATCHY_SCAN_HIT_LEN(h), h.value, h.n_ids, h.kind, h.prefix_len, 0, nullptr, 0, 0,
                       reinterpret_cast<const uint8_t*>(src.data()), (uint32_t)src.size()};
    Piece pc;
    std::string lossy;
    PayloadTexts texts{nullptr, pc, pay, v.data_offsets};
    StringSink sink{out, lossy};
    render::record_emit(r, texts, sink);
    out.pop_back();   // the '\n'
    return true;
}

int32_t Renderer::render(const ResultView& v, const Keys& k, Payloads pay, char** out, size_t* out_len, std::string& error) {
    const size_t n_hits = v.hits ? v.n_hits : 0, n_ip4 = v.ip4_hits ? v.n_ip4_hits : 0, n = n_hits + n_ip4;
    error.clear();
    if (k.sources && ((n_hits && !v.segment_of_hit) || (n_ip4 && !v.segment_of_ip4_hit))) error = "matchy_scan_result_to_ndjson_segments: the result has no segment indices";
    else if (k.with_lines && ((n_hits && !v.lines) || (n_ip4 && !v.ip4_lines))) error = "matchy_scan_result_to_ndjson_lines: the result has no line records";
    if (!error.empty()) return MATCHY_ERROR_INVALID_PARAM;
    if (source_of_ != (k.source ? k.source : "-") || source_.empty()) {
        source_of_ = k.source ? k.source : "-";
        source_ = escaped(k.source);
    }
    // the JSON text of the source of every segment that owns a record
    std::vector<std::string> seg_source;
    if (k.sources) {
        seg_source.resize(v.n_segments);
        for (size_t s = 0; s < v.n_segments; ++s) if (v.segments[s].hits) seg_source[s] = escaped(k.sources[s]);
    }
    const uint32_t flags = !k.with_lines ? 0u : k.with_input_line ? render::FLAG_LINE_NUMBERS | render::FLAG_INPUT_LINE : render::FLAG_LINE_NUMBERS;
    auto render_piece = [&](size_t i0, size_t i1, Piece& pc) {
        pc.o.reserve((i1 - i0) * 192 + 64);
        std::string lossy;
        PayloadTexts texts{&json_of_data_, pc, pay, v.data_offsets};
        StringSink sink{pc.o, lossy};
        for (size_t i = i0; i < i1; ++i) {
            const bool in_hits = i < n_hits;
            const size_t at = in_hits ? i : i - n_hits;
            const matchy_scan_hit_t h = in_hits ? v.hits[at] : matchy_scan_ip4_hit_expand(v.ip4_hits[at]);
            BlockLine bl{};
            if (v.block && !block_line_of(v, in_hits, at, h.start, bl))
                throw std::out_of_range("matchy_scan_result_to_ndjson: a record has no line in the block of hit lines");
            const uint32_t seg = !k.sources ? 0u : in_hits ? v.segment_of_hit[at] : v.segment_of_ip4_hit[at];
            if (k.sources && seg >= v.n_segments) throw std::out_of_range("matchy_scan_result_to_ndjson_segments: a segment index lies outside the table");
            const std::string& src = k.sources ? seg_source[seg] : source_;
            render::RecordIn r{v.block ? bl.hit : v.text + h.start, MATCHY_SCAN_HIT_LEN(h), h.value, h.n_ids, h.kind, h.prefix_len, flags, nullptr, 0, 0,
                               reinterpret_cast<const uint8_t*>(src.data()), (uint32_t)src.size()};
            if (flags) {
                const matchy_scan_line_t ln = in_hits ? v.lines[at] : v.ip4_lines[at];
                r.line = v.block ? bl.line : v.text + ln.line_start;
                r.line_len = v.block ? bl.line_len : ln.line_end - ln.line_start;
                r.line_number = (k.sources ? k.line_bases[seg] - v.segments[seg].line_base : k.line_base) + ln.line + 1;
            }
            render::record_emit(r, texts, sink);
        }
    };
    // One piece of the result per thread (large results only: a 256 MiB batch of a web-server log carries ~70 K matches, ~15 MB of text; one thread
    // renders ~9 M lines a second, which is less than two scanners on one GPU deliver).
    static const unsigned max_threads = [] {
        if (const char* e = getenv("MATCHY_AMD_JSON_THREADS")) return (unsigned)std::max(1, atoi(e));
        const unsigned hw = std::thread::hardware_concurrency();
        return hw >= 8 ? 4u : hw >= 4 ? 2u : 1u;
    }();
    const unsigned nt = (unsigned)std::min<size_t>(max_threads, std::max<size_t>(1, n / 16384));
    std::vector<Piece> pieces(nt);
    try {
        if (nt == 1) render_piece(0, n, pieces[0]);
        else {
            // An exception must not leave a render thread (std::terminate), and none may leave this scope while a thread is still
            // joinable: every piece catches its own, the joiner runs on every way out, the first failure is rethrown afterwards.
            std::atomic<bool> failed{false};
            std::vector<std::thread> th;
            Joiner joiner{th};
            auto guarded = [&](size_t i0, size_t i1, Piece& pc) {
                try { render_piece(i0, i1, pc); } catch (...) { failed.store(true); }
            };
            th.reserve(nt);
            for (unsigned t = 1; t < nt; ++t) th.emplace_back([&, t] { guarded(n * t / nt, n * (t + 1) / nt, pieces[t]); });
            guarded(0, n / nt, pieces[0]);
            for (auto& x : th) x.join();
            if (failed.load()) throw std::bad_alloc();
        }
        for (Piece& pc : pieces)
            for (auto& e : pc.fresh) {
                if (json_of_data_.size() > (1u << 20)) json_of_data_.clear();   // a database with millions of distinct payloads: bounded
                json_of_data_.emplace(e.first, std::move(e.second));
            }
    } catch (const std::exception& e) { error = e.what(); return MATCHY_ERROR_OUT_OF_MEMORY; }
    size_t total = 0;
    for (const Piece& pc : pieces) total += pc.o.size();
    char* buf = (char*)malloc(total + 1);
    if (!buf) { error = "matchy_scan_result_to_ndjson: out of memory"; return MATCHY_ERROR_OUT_OF_MEMORY; }
    {
        std::vector<std::thread> th;
        Joiner joiner{th};
        size_t at = 0;
        for (unsigned t = 0; t < nt; ++t) {
            char* dst = buf + at;
            at += pieces[t].o.size();
            bool spawned = false;
            if (t + 1 < nt) {
                try { th.emplace_back([dst, &pieces, t] { memcpy(dst, pieces[t].o.data(), pieces[t].o.size()); }); spawned = true; }
                catch (...) {}   // no thread to be had: copy here
            }
            if (!spawned) memcpy(dst, pieces[t].o.data(), pieces[t].o.size());
        }
    }
    buf[total] = 0;
    *out = buf; *out_len = total;
    return MATCHY_SUCCESS;
}

}  // namespace ndjson
}  // namespace mxy
