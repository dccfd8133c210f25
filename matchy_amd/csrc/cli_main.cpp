// `matchy` command line for the MI355X build: the two subcommands of the reference CLI that sit on the hot path
// (crates/matchy/src/bin/matchy.rs:78-212) — build and match — and query (bin/commands/query_cmd.rs), extract
// (bin/commands/extract_cmd.rs), inspect and validate (host only); usage() below has the synopsis of each.
// This file holds main and the small commands; `matchy match` and the description of its flags are in cli_match.cpp.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <ctime>
#include <iterator>

#include "cli_common.h"
#include "batch_reader.h"
#include "db_image.h"

using namespace mxy;

int usage() {
    fprintf(stderr,
            "usage:\n"
            "  matchy build <INPUT>... -o <FILE> [-f text|csv|json] [-t TYPE] [-d DESC] [--desc-lang LANG] [-i] [-v]\n"
            "  matchy match <DATABASE> <INPUT>... [--format json|summary] [-s] [--batch-bytes N] [--extractors LIST] [--device N | --devices LIST|all] [-j N|auto] [-f]\n"
            "               [--line-numbers] [--input-line]   (\"line_number\" / \"input_line\" in every record, computed on the GPU)\n"
            "               [--tally[=N]]   (behind the matches: one JSON line per distinct matched value with its hit count, the N most frequent; default 20,\n"
            "                                0 = all; counted on the GPU; with --format summary nothing else is printed; not with --follow)\n"
            "               [--pack-inputs]   (consecutive small files share a batch and are told apart on the GPU; same output; not with --follow)\n"
            "               [--gz-on-gpu]   (consecutive small .gz files cross the bus compressed and are inflated on the GPU, one wave per file; not with --follow)\n"
            "               [--gz-members]   (with --gz-on-gpu: a .gz file of many small members that fits one batch is inflated by one wave per member)\n"
            "               [--gz-windows]   (with --gz-on-gpu --gz-members: a multi-member .gz file larger than a batch is scanned as a chain of windows of whole members)\n"
            "               [--gz-stream-windows]   (with --gz-on-gpu --gz-pieces: a .gz file of ONE member that does not fit a batch, compressed or inflated, is scanned as a chain of windows of its stream)\n"
            "               [--gz-pieces[=BYTES]]   (with --gz-on-gpu: one large DEFLATE stream is inflated by many waves, in pieces of BYTES compressed bytes,\n"
            "                                        a power of two from 512 to 1048576; a .gz member may then be as large as a batch holds)\n"
            "               [--gather-lines]   (the lines with a match are gathered on the GPU and records are rendered from them: with --gz-on-gpu no inflated\n"
            "                                   text crosses the bus; same output; gains nothing where nearly every line matches)\n"
            "               [--render-on-gpu]   (with --format json: batches whose line numbers are known when they are submitted leave the GPU as\n"
            "                                    finished NDJSON; the others, and any the GPU refuses, are rendered on the host; same output; not with --follow)\n"
            "               [--whole-lines]   (every input line is ONE query, looked up whole like `matchy query` does a value: lists of addresses, names or\n"
            "                                  hashes; no extraction; not with --extractors, --pack-inputs, --gz-on-gpu, --gather-lines, --render-on-gpu)\n"
            "               [--encoding=utf-16le|utf-16be|auto]   (UTF-16 inputs are transcoded to UTF-8 on the GPU in front of the scan; auto: per input, by a\n"
            "                                  leading BOM, anything else is scanned as bytes; a leading BOM is skipped; offsets are those of the UTF-8 text;\n"
            "                                  not with --follow, --pack-inputs, --gz-on-gpu, --whole-lines)\n"
            "               [--unescape=percent|json|json+percent]   (%%XX and/or JSON string escapes are decoded on the GPU in front of the scan; an escape\n"
            "                                  for a line end becomes a space, so line numbers are the input's; offsets are those of the decoded text;\n"
            "                                  not with --follow, --pack-inputs, --gz-on-gpu, --whole-lines, --encoding)\n"
            "  matchy query <DATABASE> <QUERY> [-q]\n"
            "  matchy extract <INPUT>... [--format json|csv|text] [--types LIST] [--min-labels N] [-u] [-s] [--show-candidates]\n"
            "               [--render-on-gpu]   (the items of a batch are put into line order and written as json / csv / text on the GPU: one block per\n"
            "                                    batch crosses the bus in place of the item records; same output; not with --show-candidates)\n"
            "  matchy inspect <DATABASE> [-j] [-v]\n"
            "  matchy validate <DATABASE> [-l standard|strict] [-j]\n");
    return 2;
}

namespace {

int cmd_build(int argc, char** argv) {
    std::vector<std::string> inputs;
    std::string out, format = "text", dbtype, desc, lang = "en";
    bool verbose = false, case_insensitive = false;
    for (int i = 0; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&](const char* name) -> const char* { if (i + 1 >= argc) { fprintf(stderr, "error: %s needs a value\n", name); exit(2); } return argv[++i]; };
        if (a == "-o" || a == "--output") out = next("-o");
        else if (a == "-f" || a == "--format") format = next("-f");
        else if (a == "-t" || a == "--database-type") dbtype = next("-t");
        else if (a == "-d" || a == "--description") desc = next("-d");
        else if (a == "--desc-lang") lang = next("--desc-lang");
        else if (a == "-v" || a == "--verbose" || a == "--debug") verbose = true;
        else if (a == "-i" || a == "--case-insensitive") case_insensitive = true;
        else if (!a.empty() && a[0] == '-' && a != "-") { fprintf(stderr, "error: unexpected argument '%s'\n", a.c_str()); return 2; }
        else inputs.push_back(a);
    }
    if (inputs.empty() || out.empty()) return usage();
    DatabaseBuilder b(case_insensitive);
    if (!dbtype.empty()) b.set_database_type(dbtype);
    if (!desc.empty()) b.set_description(lang, desc);
    if (const char* e = getenv("MATCHY_BUILD_EPOCH")) b.set_build_epoch(strtoull(e, nullptr, 10));  // reproducible builds
    std::string err;
    if (!add_inputs(b, inputs, format, verbose, err)) { fprintf(stderr, "Error: %s\n", err.c_str()); return 1; }
    std::vector<uint8_t> blob;
    if (!b.build(blob)) { fprintf(stderr, "Error: %s\n", b.error().c_str()); return 1; }
    (void)chmod(out.c_str(), 0644);  // a previous build left the file read-only
    FILE* f = fopen(out.c_str(), "wb");
    if (!f || fwrite(blob.data(), 1, blob.size(), f) != blob.size()) { fprintf(stderr, "Error: Failed to write %s\n", out.c_str()); if (f) fclose(f); return 1; }
    fclose(f);
    (void)chmod(out.c_str(), 0444);  // the reference marks databases read-only (build_cmd.rs:15-35, 364-371)
    printf("\xE2\x9C\x93 Database built: %s\n", out.c_str());
    if (verbose) {
        const BuildStats& st = b.stats();
        printf("  IP entries: %zu, literals: %zu, globs: %zu, tree nodes: %u (%d-bit records), size: %zu bytes\n", st.ip_entries,
               st.literal_entries, st.glob_entries, st.node_count, st.record_size, blob.size());
    }
    return 0;
}

// serde_json::to_string_pretty of a compact JSON text: two spaces per level, "key": value, empty containers stay "[]" / "{}"
std::string json_pretty(const std::string& c) {
    std::string o;
    int depth = 0;
    bool in_str = false;
    auto nl = [&]() { o.push_back('\n'); o.append((size_t)depth * 2, ' '); };
    for (size_t i = 0; i < c.size(); ++i) {
        const char ch = c[i];
        if (in_str) {
            o.push_back(ch);
            if (ch == '\\' && i + 1 < c.size()) o.push_back(c[++i]);
            else if (ch == '"') in_str = false;
            continue;
        }
        switch (ch) {
            case '"': in_str = true; o.push_back(ch); break;
            case '[': case '{':
                o.push_back(ch);
                if (i + 1 < c.size() && (c[i + 1] == ']' || c[i + 1] == '}')) { o.push_back(c[++i]); break; }
                ++depth; nl();
                break;
            case ']': case '}': --depth; nl(); o.push_back(ch); break;
            case ',': o.push_back(ch); nl(); break;
            case ':': o += ": "; break;
            default: o.push_back(ch);
        }
    }
    return o;
}

// matchy query (bin/commands/query_cmd.rs:8-69): pretty JSON array on stdout, exit status 0 = found, 1 = not found
int cmd_query(int argc, char** argv) {
    std::vector<std::string> pos;
    bool quiet = false;
    for (int i = 0; i < argc; ++i) {
        std::string a = argv[i];
        if (a == "-q" || a == "--quiet") quiet = true;
        else if (a == "--") { for (++i; i < argc; ++i) pos.push_back(argv[i]); }
        else if (a.size() > 1 && a[0] == '-' && pos.size() < 1) { fprintf(stderr, "error: unexpected argument '%s'\n", a.c_str()); return 2; }
        else pos.push_back(a);
    }
    if (pos.size() != 2) return usage();
    matchy_t* db = matchy_open(pos[0].c_str());
    if (!db) { fprintf(stderr, "Error: Failed to load database: %s\n", pos[0].c_str()); return 1; }
    int32_t found = 0;
    char* js = matchy_amd_query_json(db, pos[1].c_str(), &found);
    if (!js) { fprintf(stderr, "Error: Query failed for: %s: %s\n", pos[1].c_str(), matchy_amd_last_error()); matchy_close(db); return 1; }
    if (!quiet) printf("%s\n", json_pretty(js).c_str());
    matchy_free_string(js);
    matchy_close(db);
    return found ? 0 : 1;
}

// matchy extract (bin/commands/extract_cmd.rs:40-289). The reference extracts line by line (extract_from_line,
// matchy-extractor/src/lib.rs:1471-1521: domains, IPv4, e-mails, IPv6, hashes, Bitcoin, Ethereum, Monero per line); its line
// functions are the chunk functions applied to one line, no token crosses a newline, so every batch goes through
// the GPU extractor once and the items are put back into line order here. LineScanner (bin/cli_utils.rs:9-110) trims ASCII
// whitespace from both ends of a line and skips empty lines: form feeds in those margins — whitespace for the trim, not
// a word boundary for the extractor — are turned into spaces first.
struct ExtractStats { unsigned long long lines = 0, found = 0, v4 = 0, v6 = 0, dom = 0, mail = 0, bytes = 0; };
inline bool is_ws(uint8_t c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == 0x0C; }
inline int line_rank(uint8_t t) {
    switch (t) {
        case MATCHY_ITEM_TYPE_DOMAIN: return 0;
        case MATCHY_ITEM_TYPE_IPV4: return 1;
        case MATCHY_ITEM_TYPE_EMAIL: return 2;
        case MATCHY_ITEM_TYPE_IPV6: return 3;
        case MATCHY_ITEM_TYPE_BITCOIN: return 5;
        case MATCHY_ITEM_TYPE_ETHEREUM: return 6;
        case MATCHY_ITEM_TYPE_MONERO: return 7;
        default: return 4;   // the hash types
    }
}
bool extract_batch(matchy_extractor_t* ex, uint8_t* data, size_t len, int fmt, bool show_cand, bool on_gpu, ExtractStats& st) {
    if (!len) return true;
    // line table: [start, end) of every trimmed, non-empty line (--render-on-gpu: the GPU counts the newlines itself, no table)
    std::vector<std::pair<size_t, size_t>> lines;
    for (size_t p = 0; p < len;) {
        const uint8_t* nlp = (const uint8_t*)memchr(data + p, '\n', len - p);
        size_t e = nlp ? (size_t)(nlp - data) : len, a = p, b = e;
        while (a < b && is_ws(data[a])) { if (data[a] == 0x0C) data[a] = ' '; ++a; }
        while (b > a && is_ws(data[b - 1])) { if (data[b - 1] == 0x0C) data[b - 1] = ' '; --b; }
        if (b > a) { if (!on_gpu) lines.push_back({a, b}); st.lines++; st.bytes += b - a; }
        p = e + 1;
    }
    if (on_gpu) {
        matchy_amd_extract_text_t t;
        if (matchy_amd_extractor_extract_rendered(ex, data, len, (uint32_t)fmt, &t) != MATCHY_SUCCESS) {
            fprintf(stderr, "[ERROR] extraction failed: %s\n", matchy_amd_last_error());
            return false;
        }
        if (t.status == MATCHY_AMD_EXTRACT_TEXT_OK) {
            if (t.text_len) fwrite(t.text, 1, t.text_len, stdout);
            st.found += t.n_records;
            st.v4 += t.by_type[MATCHY_ITEM_TYPE_IPV4]; st.v6 += t.by_type[MATCHY_ITEM_TYPE_IPV6];
            st.dom += t.by_type[MATCHY_ITEM_TYPE_DOMAIN]; st.mail += t.by_type[MATCHY_ITEM_TYPE_EMAIL];
            return true;
        }
        // the GPU refused the batch: the host path prints it; its lines are counted already
        ExtractStats host;
        if (!extract_batch(ex, data, len, fmt, false, false, host)) return false;
        st.found += host.found; st.v4 += host.v4; st.v6 += host.v6; st.dom += host.dom; st.mail += host.mail;
        return true;
    }
    matchy_matches_t m;
    memset(&m, 0, sizeof(m));
    if (matchy_extractor_extract_chunk(ex, data, len, &m) != MATCHY_SUCCESS) {
        fprintf(stderr, "[ERROR] extraction failed: %s\n", matchy_amd_last_error());
        return false;
    }
    struct It { size_t line; int rank; size_t idx; };
    std::vector<It> its(m.count);
    for (size_t i = 0; i < m.count; ++i) {
        const size_t s = m.items[i].start;
        // the trimmed line that holds position s
        size_t lo = 0, hi = lines.size();
        while (lo < hi) { size_t mid = (lo + hi) / 2; if (lines[mid].second <= s) lo = mid + 1; else hi = mid; }
        its[i] = It{lo, line_rank(m.items[i].item_type), i};
    }
    std::sort(its.begin(), its.end(), [&](const It& a, const It& b) {
        if (a.line != b.line) return a.line < b.line;
        if (a.rank != b.rank) return a.rank < b.rank;
        return m.items[a.idx].start < m.items[b.idx].start;
    });
    std::string out;
    for (const It& it : its) {
        const matchy_match_t& mt = m.items[it.idx];
        const std::string text((const char*)data + mt.start, mt.end - mt.start);
        std::string tname = matchy_item_type_name(mt.item_type);
        if (show_cand) {
            const size_t ls = it.line < lines.size() ? lines[it.line].first : 0;
            fprintf(stderr, "[CANDIDATE] %s at %zu-%zu: %s\n", tname.c_str(), (size_t)mt.start - ls, (size_t)mt.end - ls, text.c_str());
        }
        for (char& ch : tname) ch = (char)tolower((unsigned char)ch);
        out.clear();
        if (fmt == 0) {
            out += "{\"type\":\"" + tname + "\",\"value\":\"";
            for (char ch : text) { if (ch == '\\') out += "\\\\"; else if (ch == '"') out += "\\\""; else out.push_back(ch); }
            out += "\"}\n";
        } else if (fmt == 1) {
            out += tname + ",\"";
            for (char ch : text) { if (ch == '"') out += "\"\""; else out.push_back(ch); }
            out += "\"\n";
        } else {
            out += text; out.push_back('\n');
        }
        fwrite(out.data(), 1, out.size(), stdout);
        st.found++;
        if (mt.item_type == MATCHY_ITEM_TYPE_IPV4) st.v4++;
        else if (mt.item_type == MATCHY_ITEM_TYPE_IPV6) st.v6++;
        else if (mt.item_type == MATCHY_ITEM_TYPE_DOMAIN) st.dom++;
        else if (mt.item_type == MATCHY_ITEM_TYPE_EMAIL) st.mail++;
    }
    matchy_matches_free(&m);
    return true;
}

int cmd_extract(int argc, char** argv) {
    std::vector<std::string> inputs;
    std::string format = "json", types;
    bool have_types = false, unique = false, stats = false, show_cand = false, on_gpu = false;
    uint32_t min_labels = 2;
    size_t batch_bytes = (size_t)256 << 20;
    for (int i = 0; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&](const char* name) -> const char* { if (i + 1 >= argc) { fprintf(stderr, "error: %s needs a value\n", name); exit(2); } return argv[++i]; };
        auto eqval = [&](const char* name, std::string& out) {
            size_t n = strlen(name);
            if (a.compare(0, n, name) != 0) return false;
            if (a.size() == n) { out = next(name); return true; }
            if (a[n] == '=') { out = a.substr(n + 1); return true; }
            return false;
        };
        std::string v;
        if (eqval("--format", v)) format = v;
        else if (eqval("--types", v)) { types = v; have_types = true; }
        else if (eqval("--min-labels", v)) min_labels = (uint32_t)strtoul(v.c_str(), nullptr, 10);
        else if (eqval("--batch-bytes", v)) { size_t b = strtoull(v.c_str(), nullptr, 10); if (b >= 4096) batch_bytes = b; }
        else if (a == "--no-boundaries") { fprintf(stderr, "Error: --no-boundaries is not supported by this build\n"); return 1; }
        else if (a == "-u" || a == "--unique") unique = true;
        else if (a == "-s" || a == "--stats") stats = true;
        else if (a == "--show-candidates") show_cand = true;
        else if (a == "--render-on-gpu") on_gpu = true;
        else if (a.size() > 1 && a[0] == '-') { fprintf(stderr, "error: unexpected argument '%s'\n", a.c_str()); return 2; }
        else inputs.push_back(a);
    }
    if (inputs.empty()) return usage();
    if (on_gpu && show_cand) { fprintf(stderr, "Error: --show-candidates prints every item on the host and cannot be combined with --render-on-gpu\n"); return 1; }
    for (char& ch : format) ch = (char)tolower((unsigned char)ch);
    const int fmt = format == "json" ? 0 : format == "csv" ? 1 : format == "text" ? 2 : -1;
    if (fmt < 0) { fprintf(stderr, "Error: Invalid format '%s', expected: json, csv, or text\n", format.c_str()); return 1; }
    bool v4 = true, v6 = true, dom = true, mail = true;
    if (have_types) {
        v4 = v6 = dom = mail = false;
        std::string low = types;
        for (char& ch : low) ch = (char)tolower((unsigned char)ch);
        std::stringstream ss(low);
        std::string part;
        while (std::getline(ss, part, ',')) {
            part = trim(part);
            if (part == "ipv4" || part == "ip4") v4 = true;
            else if (part == "ipv6" || part == "ip6") v6 = true;
            else if (part == "domain" || part == "domains") dom = true;
            else if (part == "email" || part == "emails") mail = true;
            else if (part == "ip") v4 = v6 = true;
            else if (part == "all") v4 = v6 = dom = mail = true;
            else { fprintf(stderr, "Error: Unknown extraction type '%s', expected: ipv4, ipv6, ip, domain, email, all\n", part.c_str()); return 1; }
        }
        if (!v4 && !v6 && !dom && !mail) { fprintf(stderr, "Error: At least one extraction type must be enabled\n"); return 1; }
    }
    // the command only switches these four; hashes and the crypto-address extractors keep the builder's default (on)
    uint32_t flags = MATCHY_EXTRACT_HASHES | MATCHY_EXTRACT_BITCOIN | MATCHY_EXTRACT_ETHEREUM | MATCHY_EXTRACT_MONERO;
    if (v4) flags |= MATCHY_EXTRACT_IPV4;
    if (v6) flags |= MATCHY_EXTRACT_IPV6;
    if (dom) flags |= MATCHY_EXTRACT_DOMAINS;
    if (mail) flags |= MATCHY_EXTRACT_EMAILS;
    matchy_extractor_t* ex = matchy_amd_extractor_create(flags, min_labels);
    if (!ex) { fprintf(stderr, "Error: Failed to create pattern extractor: %s\n", matchy_amd_last_error()); return 1; }
    if (stats) {
        std::string en;
        for (auto& pr : {std::make_pair(v4, "IPv4"), std::make_pair(v6, "IPv6"), std::make_pair(dom, "domains"), std::make_pair(mail, "emails")})
            if (pr.first) { if (!en.empty()) en += ", "; en += pr.second; }
        fprintf(stderr, "[INFO] Extracting: %s\n", en.c_str());
        if (dom) fprintf(stderr, "[INFO] Min domain labels: %u\n", min_labels);
        fprintf(stderr, "[INFO] Word boundaries: true\n[INFO] Unique mode: %s\n", unique ? "true" : "false");
    }
    const auto t0 = std::chrono::steady_clock::now();
    ExtractStats st;
    // --unique (extract_cmd.rs:133, 241-246: a set of every text printed): the handle keeps the set on the GPU and returns first occurrences only
    if (unique) matchy_amd_extractor_set_unique(ex, true);
    if (fmt == 1) fputs("type,value\n", stdout);
    bool ok = true;
    for (const std::string& path : inputs) {
        int fd = path == "-" ? 0 : open(path.c_str(), O_RDONLY);
        if (fd < 0) { fprintf(stderr, "Error: Failed to open file: %s\n", path.c_str()); ok = false; break; }
        const StreamEnd e = read_batches([&](void* p, size_t n) { return read(fd, p, n); }, batch_bytes, [&](Bytes&& data, size_t len, uint64_t) {
            return extract_batch(ex, data.get(), len, fmt, show_cand, on_gpu, st);
        });
        if (e == StreamEnd::FAILED) fprintf(stderr, "Error: read failed on %s: %s\n", path.c_str(), strerror(errno));
        ok = e == StreamEnd::DONE;
        if (fd) close(fd);
        if (!ok) break;
    }
    fflush(stdout);
    matchy_extractor_free(ex);
    if (!ok) return 1;
    if (stats) {
        const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        fprintf(stderr, "\n[INFO] === Extraction Complete ===\n[INFO] Lines processed: %s\n[INFO] Patterns found: %s\n", fmt_num(st.lines).c_str(), fmt_num(st.found).c_str());
        if (v4 && st.v4) fprintf(stderr, "[INFO]   IPv4: %s\n", fmt_num(st.v4).c_str());
        if (v6 && st.v6) fprintf(stderr, "[INFO]   IPv6: %s\n", fmt_num(st.v6).c_str());
        if (dom && st.dom) fprintf(stderr, "[INFO]   Domains: %s\n", fmt_num(st.dom).c_str());
        if (mail && st.mail) fprintf(stderr, "[INFO]   Emails: %s\n", fmt_num(st.mail).c_str());
        fprintf(stderr, "[INFO] Throughput: %.2f MB/s\n[INFO] Total time: %.2fs\n", secs > 0 ? (double)st.bytes / 1e6 / secs : 0.0, secs);
    }
    return 0;
}

// matchy inspect (bin/commands/inspect_cmd.rs:10-119): what the file holds, from its metadata; no GPU involved
bool meta_uint_of(const DataValue& m, const char* key, unsigned long long& out) {
    if (m.type != DataValue::MAP) return false;
    auto it = m.map.find(key);
    if (it == m.map.end()) return false;
    const DataValue& v = it->second;
    if (v.type == DataValue::UINT16 || v.type == DataValue::UINT32 || v.type == DataValue::UINT64) { out = v.u; return true; }
    return false;
}
std::string fmt_unix_time(unsigned long long ts) {   // bin/cli_utils.rs:255-283
    time_t t = (time_t)ts;
    struct tm g;
    gmtime_r(&t, &g);
    char b[64];
    snprintf(b, sizeof(b), "%04d-%02d-%02d %02d:%02d:%02d UTC", g.tm_year + 1900, g.tm_mon + 1, g.tm_mday, g.tm_hour, g.tm_min, g.tm_sec);
    return b;
}
std::string fmt_data_value(const DataValue& v, const std::string& indent) {   // bin/cli_utils.rs:322-364
    std::string o;
    switch (v.type) {
        case DataValue::STRING: return "\"" + v.str + "\"";
        case DataValue::MAP:
            if (v.map.empty()) return "{}";
            o = "{\n";
            for (auto& kv : v.map) o += indent + "  " + kv.first + ": " + fmt_data_value(kv.second, indent + "  ") + ",\n";
            return o + indent + "}";
        case DataValue::ARRAY:
            if (v.arr.empty()) return "[]";
            o = "[";
            for (size_t i = 0; i < v.arr.size(); ++i) { if (i) o += ", "; o += fmt_data_value(v.arr[i], indent); }
            return o + "]";
        default: { std::string j; to_json(v, j); return j; }
    }
}
int cmd_inspect(int argc, char** argv) {
    std::vector<std::string> pos;
    bool json = false, verbose = false;
    for (int i = 0; i < argc; ++i) {
        std::string a = argv[i];
        if (a == "-j" || a == "--json") json = true;
        else if (a == "-v" || a == "--verbose") verbose = true;
        else if (a.size() > 1 && a[0] == '-') { fprintf(stderr, "error: unexpected argument '%s'\n", a.c_str()); return 2; }
        else pos.push_back(a);
    }
    if (pos.size() != 1) return usage();
    std::vector<uint8_t> bytes;
    {
        std::ifstream f(pos[0], std::ios::binary);
        if (!f) { fprintf(stderr, "Error: Failed to load database: %s\n", pos[0].c_str()); return 1; }
        bytes.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    }
    DbImage img;
    std::string err;
    if (!img.open(std::move(bytes), err)) { fprintf(stderr, "Error: Failed to load database: %s: %s\n", pos[0].c_str(), err.c_str()); return 1; }
    // counts as Database::ip_count / literal_count / glob_count report them (database.rs:1147-1210): metadata first
    unsigned long long ipc = 0, litc = 0, globc = 0;
    if (!meta_uint_of(img.metadata, "ip_entry_count", ipc)) (void)meta_uint_of(img.metadata, "node_count", ipc);
    (void)meta_uint_of(img.metadata, "literal_entry_count", litc);
    if (!meta_uint_of(img.metadata, "glob_entry_count", globc)) globc = img.pattern_count;
    const bool has_string = img.has_literal || img.has_glob;
    if (json) {
        std::string o = "{\"file\":";
        auto esc = [&](const std::string& x) { std::string q; to_json(DataValue::String(x), q); return q; };
        o += esc(pos[0]) + ",\"format\":" + esc(img.format_name());
        o += std::string(",\"glob_count\":") + std::to_string(globc) + ",\"has_glob_data\":" + (img.has_glob ? "true" : "false");
        o += std::string(",\"has_ip_data\":") + (img.has_ip ? "true" : "false") + ",\"has_literal_data\":" + (img.has_literal ? "true" : "false");
        o += std::string(",\"has_string_data\":") + (has_string ? "true" : "false") + ",\"ip_count\":" + std::to_string(ipc) + ",\"literal_count\":" + std::to_string(litc);
        if (img.metadata.type == DataValue::MAP) { o += ",\"metadata\":"; to_json(img.metadata, o); }
        o += "}";
        printf("%s\n", json_pretty(o).c_str());
        return 0;
    }
    printf("Database: %s\n", pos[0].c_str());
    printf("Format:   %s\n\n", ipc > 0 && (litc > 0 || globc > 0) ? "Combined IP+String database" : ipc > 0 ? "IP database" : (litc > 0 || globc > 0) ? "String database" : "Empty database");
    printf("Capabilities:\n");
    if (ipc > 0) printf("  IP lookups:      \xE2\x9C\x93\n    Entries:       %llu\n", ipc);
    else printf("  IP lookups:      \xE2\x9C\x97\n");
    printf("  String lookups:  %s\n", has_string ? "\xE2\x9C\x93" : "\xE2\x9C\x97");
    if (img.has_literal) printf("    Literals:      \xE2\x9C\x93 (%llu strings)\n", litc);
    if (img.has_glob) printf("    Globs:         \xE2\x9C\x93 (%llu patterns)\n", globc);
    if (img.metadata.type == DataValue::MAP) {
        printf("\nMetadata:\n");
        auto it = img.metadata.map.find("database_type");
        if (it != img.metadata.map.end() && it->second.type == DataValue::STRING) printf("  Database type:   %s\n", it->second.str.c_str());
        it = img.metadata.map.find("description");
        if (it != img.metadata.map.end() && it->second.type == DataValue::MAP) {
            printf("  Description:\n");
            for (auto& kv : it->second.map) if (kv.second.type == DataValue::STRING) printf("    %s: %s\n", kv.first.c_str(), kv.second.str.c_str());
        }
        unsigned long long v;
        if (meta_uint_of(img.metadata, "build_epoch", v)) printf("  Build time:      %s (%llu)\n", fmt_unix_time(v).c_str(), v);
        if (meta_uint_of(img.metadata, "ip_version", v)) printf("  IP version:      IPv%llu\n", v);
        if (verbose) printf("\nFull metadata:\n%s\n", fmt_data_value(img.metadata, "  ").c_str());
    }
    return 0;
}

// matchy validate (bin/commands/validate_cmd.rs): the structural checks of matchy_validate = DbImage::check_structure, the same
// checks every matchy_open runs before a file is uploaded (headers, metadata, section bounds, every pointer the kernels follow:
// IP data records, literal-hash strings, wildcard / pattern / glob-segment arrays, the reachable Aho-Corasick nodes). Both
// levels run the same checks here; exit status 0 = valid. The reference's detailed statistics block is not reproduced.
int cmd_validate(int argc, char** argv) {
    std::vector<std::string> pos;
    std::string level = "strict";
    bool json = false;
    for (int i = 0; i < argc; ++i) {
        std::string a = argv[i];
        if (a == "-j" || a == "--json") json = true;
        else if (a == "-v" || a == "--verbose") {}
        else if (a == "-l" || a == "--level") { if (i + 1 >= argc) return usage(); level = argv[++i]; }
        else if (a.compare(0, 8, "--level=") == 0) level = a.substr(8);
        else if (a.size() > 1 && a[0] == '-') { fprintf(stderr, "error: unexpected argument '%s'\n", a.c_str()); return 2; }
        else pos.push_back(a);
    }
    if (pos.size() != 1) return usage();
    for (char& ch : level) ch = (char)tolower((unsigned char)ch);
    if (level != "standard" && level != "strict") { fprintf(stderr, "Error: Invalid validation level: '%s'. Must be: standard or strict\n", level.c_str()); return 1; }
    char* msg = nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    const int32_t rc = matchy_validate(pos[0].c_str(), level == "strict" ? MATCHY_VALIDATION_STRICT : MATCHY_VALIDATION_STANDARD, &msg);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    const bool valid = rc == MATCHY_SUCCESS;
    if (json) {
        std::string o = "{\"database\":";
        std::string q;
        to_json(DataValue::String(pos[0]), q);
        o += q + ",\"duration_ms\":" + std::to_string((long long)ms) + ",\"errors\":[";
        if (!valid) { q.clear(); to_json(DataValue::String(msg ? msg : "validation failed"), q); o += q; }
        o += std::string("],\"is_valid\":") + (valid ? "true" : "false") + ",\"validation_level\":\"" + level + "\"}";
        printf("%s\n", json_pretty(o).c_str());
    } else {
        printf("Validating: %s\nLevel:      %s\n\n", pos[0].c_str(), level.c_str());
        if (!valid) printf("\xE2\x9D\x8C ERRORS (1):\n  \xE2\x80\xA2 %s\n\n", msg ? msg : "validation failed");
        printf("%s\n", valid ? "\xE2\x9C\x85 VALIDATION PASSED (structural checks: every offset the readers follow lies inside its section)" : "\xE2\x9D\x8C VALIDATION FAILED");
    }
    if (msg) matchy_free_string(msg);
    return valid ? 0 : 1;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return usage();
    std::string cmd = argv[1];
    if (cmd == "build") return cmd_build(argc - 2, argv + 2);
    if (cmd == "match") return cmd_match(argc - 2, argv + 2);
    if (cmd == "query") return cmd_query(argc - 2, argv + 2);
    if (cmd == "extract") return cmd_extract(argc - 2, argv + 2);
    if (cmd == "inspect") return cmd_inspect(argc - 2, argv + 2);
    if (cmd == "validate") return cmd_validate(argc - 2, argv + 2);
    if (cmd == "--version" || cmd == "-V" || cmd == "version") { printf("matchy %s (MI355X build)\n", matchy_version()); return 0; }
    return usage();
}
