// `matchy` command line for the MI355X build: the two subcommands of the reference CLI that sit on the hot path
// (crates/matchy/src/bin/matchy.rs:78-212):
//
//   matchy build <INPUT>... -o <FILE> [-f text|csv|json] [-t TYPE] [-d DESC] [--desc-lang LANG] [-i] [-v]
//   matchy match <DATABASE> <INPUT>... [--format json|summary] [-s] [--batch-bytes N] [--extractors LIST] [--device N | --devices LIST|all]
//   matchy query <DATABASE> <QUERY> [-q]                                  (bin/commands/query_cmd.rs)
//   matchy extract <INPUT>... [--format json|csv|text] [--types LIST] [--min-labels N] [-u] [-s] [--show-candidates]
//                                                                          (bin/commands/extract_cmd.rs)
//   matchy inspect <DATABASE> [-j] [-v]          matchy validate <DATABASE> [-l standard|strict] [-j]      (host only)
//
// `match` prints one JSON object per match on stdout (same records as the reference's parallel path,
// match_processor/parallel.rs:297-369: sorted keys, timestamp "0.000") and, with -s, the [INFO] statistics block on
// stderr (commands/match_cmd.rs:514-581). Every batch is scanned on the GPU through the C ABI (matchy_scanner_scan);
// there is no CPU scan path. Flags that only tune the reference's CPU thread pool (-j, --readers, --cache-size, -p,
// --debug-routing) are accepted and ignored; .gz inputs are decompressed on the host (zlib); -f/--follow polls the files.
// --tally[=N] adds, behind the match records, {"count","item_type","matched_text","result"} per distinct matched value (tally.hip).
// --pack-inputs reads consecutive small input files into shared batches (input_packer.h) and scans each as one batch of segments
// (segments.hip): the output is byte for byte what it is without the flag.
// --gz-on-gpu sends runs of consecutive small .gz inputs to the GPU compressed (matchy_multi_scanner_submit_gz, inflate.hip): one wave
// per file inflates them into the segments of one batch. A file the GPU does not accept (a second member, a damaged stream) is read the
// old way right behind its pack, so it is scanned or reported exactly as without the flag; only its place in the output moves.
// --gz-members (with --gz-on-gpu) extends the packs to .gz files of many small members that fit one batch
// (matchy_multi_scanner_submit_gz_files): one wave per member, the file is one segment, the verdict is per file.
// --gz-windows (with both) extends that to multi-member .gz files LARGER than a batch: the mapped file goes out as a chain of windows of
// whole members (matchy_multi_scanner_submit_gz_window), one at a time; every window hands the partial line behind its last '\n' to the next.
#include <fcntl.h>
#include <signal.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <fstream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/matchy_amd.h"
#include "data_codec.h"
#include "db_builder.h"
#include "batch_reader.h"
#include "db_image.h"
#include "gz_plan.h"
#include "input_packer.h"

using namespace mxy;

namespace {

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
            "               [--gather-lines]   (the lines with a match are gathered on the GPU and records are rendered from them: with --gz-on-gpu no inflated\n"
            "                                   text crosses the bus; same output; gains nothing where nearly every line matches)\n"
            "               [--render-on-gpu]   (with --format json: batches whose line numbers are known when they are submitted leave the GPU as\n"
            "                                    finished NDJSON; the others, and any the GPU refuses, are rendered on the host; same output; not with --follow)\n"
            "               [--whole-lines]   (every input line is ONE query, looked up whole like `matchy query` does a value: lists of addresses, names or\n"
            "                                  hashes; no extraction; not with --extractors, --pack-inputs, --gz-on-gpu, --gather-lines, --render-on-gpu)\n"
            "  matchy query <DATABASE> <QUERY> [-q]\n"
            "  matchy extract <INPUT>... [--format json|csv|text] [--types LIST] [--min-labels N] [-u] [-s] [--show-candidates]\n"
            "  matchy inspect <DATABASE> [-j] [-v]\n"
            "  matchy validate <DATABASE> [-l standard|strict] [-j]\n");
    return 2;
}

bool ends_with_ci(const std::string& s, const char* suf) {
    size_t n = strlen(suf);
    if (s.size() < n) return false;
    for (size_t i = 0; i < n; ++i) if (tolower((unsigned char)s[s.size() - n + i]) != suf[i]) return false;
    return true;
}

std::string fmt_num(unsigned long long v) {  // 1234567 -> "1,234,567" (bin/cli_utils.rs:143-153)
    std::string s = std::to_string(v), out;
    for (size_t i = 0; i < s.size(); ++i) {
        if (i && (s.size() - i) % 3 == 0) out.push_back(',');
        out.push_back(s[i]);
    }
    return out;
}

std::string trim(const std::string& s) {
    size_t a = 0, b = s.size();
    while (a < b && isspace((unsigned char)s[a])) ++a;
    while (b > a && isspace((unsigned char)s[b - 1])) --b;
    return s.substr(a, b - a);
}

// One CSV record (RFC 4180 quoting as the `csv` crate reads it by default: quotes, doubled quotes, embedded newlines).
bool read_csv_record(std::istream& in, std::vector<std::string>& out) {
    out.clear();
    std::string cell;
    bool quoted = false, any = false;
    int ch;
    while ((ch = in.get()) != EOF) {
        any = true;
        if (quoted) {
            if (ch == '"') {
                if (in.peek() == '"') { cell.push_back('"'); in.get(); }
                else quoted = false;
            } else cell.push_back((char)ch);
        } else if (ch == '"' && cell.empty()) quoted = true;
        else if (ch == ',') { out.push_back(cell); cell.clear(); }
        else if (ch == '\n') { if (!cell.empty() && cell.back() == '\r') cell.pop_back(); out.push_back(cell); return true; }
        else cell.push_back((char)ch);
    }
    if (!any) return false;
    out.push_back(cell);
    return true;
}

// CSV cell typing of the reference CLI (commands/build_cmd.rs:226-236): i64 -> Int32 (truncating), u64 -> Uint64,
// f64 -> Double, true/false -> Bool, else String.
DataValue csv_value(const std::string& v) {
    errno = 0;
    char* end = nullptr;
    if (!v.empty() && !isspace((unsigned char)v[0])) {
        long long i = strtoll(v.c_str(), &end, 10);
        if (errno == 0 && end && *end == 0 && (isdigit((unsigned char)v[0]) || ((v[0] == '-' || v[0] == '+') && v.size() > 1 && isdigit((unsigned char)v[1]))))
            return DataValue::Int32((int32_t)i);
        errno = 0;
        if (isdigit((unsigned char)v[0]) || (v[0] == '+' && v.size() > 1)) {
            unsigned long long u = strtoull(v.c_str(), &end, 10);
            if (errno == 0 && end && *end == 0) return DataValue::Uint64(u);
        }
        errno = 0;
        double f = strtod(v.c_str(), &end);
        if (errno == 0 && end && *end == 0 && end != v.c_str()) {
            // Rust's f64::from_str accepts decimal / exponent forms, "inf", "infinity", "nan" (any case); it has no hex floats
            bool hexish = v.find('x') != std::string::npos || v.find('X') != std::string::npos;
            if (!hexish) return DataValue::Double(f);
        }
    }
    if (v == "true" || v == "false") return DataValue::Bool(v == "true");
    return DataValue::String(v);
}

bool add_inputs(DatabaseBuilder& b, const std::vector<std::string>& inputs, const std::string& format, bool verbose, std::string& err) {
    size_t total = 0;
    for (const std::string& path : inputs) {
        std::ifstream in(path, std::ios::binary);
        if (!in) { err = "Failed to open input file: " + path; return false; }
        if (format == "text") {
            std::string line;
            bool first = true;
            while (std::getline(in, line)) {
                if (first) {
                    first = false;
                    size_t commas = 0;
                    for (char c : line) commas += c == ',';
                    if (commas >= 3)
                        fprintf(stderr, "Warning: %s looks like CSV but you specified --format text.\nIf this is a CSV file, use --format csv instead.\n", path.c_str());
                }
                std::string entry = trim(line);
                if (entry.empty() || entry[0] == '#') continue;
                if (!b.add_entry(entry, DataValue::Map())) { err = "Failed to add entry '" + entry + "': " + b.error(); return false; }
                ++total;
            }
        } else if (format == "csv") {
            std::vector<std::string> hdr, rec;
            if (!read_csv_record(in, hdr)) { err = "Failed to read CSV headers"; return false; }
            int entry_col = -1;
            for (size_t i = 0; i < hdr.size(); ++i) if (hdr[i] == "entry" || hdr[i] == "key") { entry_col = (int)i; break; }
            if (entry_col < 0) {
                err = "CSV must have an 'entry' or 'key' column. Found headers: ";
                for (size_t i = 0; i < hdr.size(); ++i) err += (i ? ", " : "") + hdr[i];
                return false;
            }
            size_t row = 1;
            while (read_csv_record(in, rec)) {
                ++row;
                if (rec.size() == 1 && rec[0].empty()) continue;  // blank line
                if ((size_t)entry_col >= rec.size()) { err = "Missing entry column at row " + std::to_string(row); return false; }
                DataValue data = DataValue::Map();
                for (size_t i = 0; i < hdr.size() && i < rec.size(); ++i)
                    if ((int)i != entry_col && !rec[i].empty()) data.map[hdr[i]] = csv_value(rec[i]);
                if (!b.add_entry(rec[entry_col], data)) {
                    err = "Failed to add entry '" + rec[entry_col] + "' at row " + std::to_string(row) + ": " + b.error();
                    return false;
                }
                ++total;
            }
        } else if (format == "json") {
            // [{"key": "...", "data": {...}}, ...] with the CLI's number typing (bin/cli_utils.rs:203-236)
            std::stringstream ss;
            ss << in.rdbuf();
            std::string text = ss.str(), perr;
            DataValue doc;
            if (!parse_json(text.data(), text.size(), NumberTyping::CLI, doc, perr)) { err = "Failed to parse JSON: " + perr; return false; }
            if (doc.type != DataValue::ARRAY) { err = "Failed to parse JSON: expected an array of {key, data} objects"; return false; }
            for (size_t i = 0; i < doc.arr.size(); ++i) {
                const DataValue& item = doc.arr[i];
                auto k = item.type == DataValue::MAP ? item.map.find("key") : item.map.end();
                if (item.type != DataValue::MAP || k == item.map.end() || k->second.type != DataValue::STRING) {
                    err = "Missing 'key' field at index " + std::to_string(i);
                    return false;
                }
                DataValue data = DataValue::Map();
                auto d = item.map.find("data");
                if (d != item.map.end()) {
                    if (d->second.type != DataValue::MAP) { err = "Expected JSON object for data at index " + std::to_string(i); return false; }
                    data = d->second;
                }
                if (!b.add_entry(k->second.str, data)) {
                    err = "Failed to add entry '" + k->second.str + "' at index " + std::to_string(i) + ": " + b.error();
                    return false;
                }
                ++total;
            }
        } else {
            err = "Unknown format: " + format + ". Use 'text', 'csv' or 'json'";
            return false;
        }
    }
    if (verbose) printf("  Total: %zu entries\n", total);
    return true;
}

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

// --extractors=ip,domain / -crypto,-hash ... (bin/matchy.rs:124-131): returns the MATCHY_EXTRACT_* mask, 0 = auto
bool parse_extractors(const std::string& spec, uint32_t auto_mask, uint32_t& mask, std::string& err) {
    struct { const char* name; uint32_t bits; } names[] = {
        {"ipv4", MATCHY_EXTRACT_IPV4}, {"ipv6", MATCHY_EXTRACT_IPV6}, {"ip", MATCHY_EXTRACT_IPV4 | MATCHY_EXTRACT_IPV6}, {"ips", MATCHY_EXTRACT_IPV4 | MATCHY_EXTRACT_IPV6},
        {"domain", MATCHY_EXTRACT_DOMAINS}, {"domains", MATCHY_EXTRACT_DOMAINS}, {"email", MATCHY_EXTRACT_EMAILS}, {"emails", MATCHY_EXTRACT_EMAILS},
        {"hash", MATCHY_EXTRACT_HASHES}, {"hashes", MATCHY_EXTRACT_HASHES}, {"bitcoin", MATCHY_EXTRACT_BITCOIN}, {"ethereum", MATCHY_EXTRACT_ETHEREUM},
        {"monero", MATCHY_EXTRACT_MONERO}, {"crypto", MATCHY_EXTRACT_BITCOIN | MATCHY_EXTRACT_ETHEREUM | MATCHY_EXTRACT_MONERO},
    };
    uint32_t enable = 0, disable = 0;
    std::stringstream ss(spec);
    std::string tok;
    while (std::getline(ss, tok, ',')) {
        tok = trim(tok);
        if (tok.empty()) continue;
        bool neg = tok[0] == '-';
        std::string n = neg ? tok.substr(1) : tok;
        for (auto& c : n) c = (char)tolower((unsigned char)c);
        uint32_t bits = 0;
        for (auto& e : names) if (n == e.name) bits = e.bits;
        if (!bits) { err = "Unknown extractor: " + n; return false; }
        (neg ? disable : enable) |= bits;
    }
    mask = (enable ? enable : auto_mask) & ~disable;
    return true;
}

struct Totals {
    unsigned long long lines = 0, lines_with_matches = 0, matches = 0, candidates = 0, bytes = 0;
};

// --gz-on-gpu: one file of a gz pack, and the statuses of a pack's members (MATCHY_GZ_*) on their way from the worker that scanned the
// pack to the reader, which reads the members that failed the old way before it submits anything else
// --gz-members: isize is the sum over the file's members, of which there are `members`
struct GzFile { size_t input; uint64_t offset; uint32_t len, isize; uint32_t members = 1; };
struct GzVerdict {
    std::mutex mu;
    std::condition_variable cv;
    bool done = false;
    std::vector<int32_t> status;   // empty with done set: the pack was not scanned at all, every member is read the old way
    // --gz-windows: MATCHY_WINDOW_*, the carry for the next window and the bytes of the file this window consumed; written before set()
    int32_t window_status = MATCHY_WINDOW_OK;
    std::vector<uint8_t> carry;
    uint64_t bytes = 0;
    void set(const int32_t* st, size_t n) {
        { std::lock_guard<std::mutex> lk(mu); if (done) return; status.assign(st, st + n); done = true; }
        cv.notify_all();
    }
    void wait() { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return done; }); }
};

// ---- `matchy match`: reader -> batches -> one worker per device entry -> ordered printer
// The pipeline itself is the library's (matchy_multi_scanner_*: one worker thread and scanner per device entry, batches handed out in
// sequence, results taken back in sequence — processing/parallel.rs:494-505 behind the C ABI). What stays here is what belongs to
// the command line: the reader cuts every input into newline-aligned batches (FileReader::next_batch, processing/mod.rs:206-251;
// regular files are mapped, .gz / stdin are read), the batch hook renders a batch's matches on the worker that scanned it, and the
// printer emits the rendered batches in sequence order, so the output is the same for every device list (line blocks
// are independent, the database is replicated, the host gathers the hit records and sums the counters; no collective).
// `ptr` points into `own` (inputs that are read: stdin, .gz) or into a file mapping that outlives the batch
struct Batch { size_t input = 0; Bytes own; const uint8_t* ptr = nullptr; size_t len = 0; bool mapped = false;
               const void* reg = nullptr;   // reg: page range of a batch the reader pinned ahead of the scan (unpinned by the worker)
               // --pack-inputs: the files of a pack, one segment each (empty: an ordinary batch of `input`), and the newlines the packer added
               std::vector<PackedInput> pack; size_t appended = 0;
               // --gz-on-gpu: the gzip files of a gz pack (`ptr` holds them compressed, end to end), one segment each, and where the
               // reader waits for the verdict on them
               std::vector<GzFile> gz; std::shared_ptr<GzVerdict> verdict;
               // --gz-windows: the batch is one window of the file gz[0] (`ptr` holds its whole members, in the file's mapping) behind `carry`;
               // it is ONE segment like a pack of one file, but its lines count on from those of the windows in front
               bool window = false, window_last = false; std::vector<uint8_t> carry; uint32_t carry_cap = 0;
               bool armed = false; };   // --render-on-gpu: the batch was submitted with matchy_multi_scanner_set_render
// what a batch contributes to the output: `text` / `text_len` is the buffer matchy_scan_result_to_ndjson returned (written to stdout as
// it is and released by the printer: 200 bytes per match are not copied again on the way), `out` what --follow builds from it
struct Done {
    std::string out; char* text = nullptr; size_t text_len = 0; Totals t; bool ok = true; size_t input = 0;
    bool skip = false;   // nothing of the batch is printed from its result: its inputs are read again the old way
    Done() = default;
    Done(const Done&) = delete;
    Done& operator=(const Done&) = delete;
    ~Done() { if (text) matchy_free_string(text); }
};
// all of a buffer to stdout, past stdio (a gigabyte of NDJSON per ten gigabytes of log need not pass through its buffer)
static void write_all_stdout(const char* p, size_t n) {
    fflush(stdout);
    while (n) {
        const ssize_t w = write(1, p, n);
        if (w < 0) { if (errno == EINTR) continue; return; }
        p += w; n -= (size_t)w;
    }
}

struct MatchPipeline {
    matchy_multi_scanner_t* ms = nullptr;
    std::mutex mu;
    size_t submitted = 0;
    std::atomic<bool> reader_done{false};
    bool json = true;
    std::vector<std::string> sources;
    // --line-numbers / --input-line: the scanners run with line context. "Lines with matches" is the device's count, and the records
    // carry "line_number" (1-based per input) — which needs the number of lines in front of the batch, known only in sequence order:
    // such batches are rendered by the ordered printer (line_base: '\n' bytes of the input's earlier batches; batches end at newlines),
    // not by the batch hook.
    bool line_ctx = false, input_line = false;
    // --gather-lines: the scanners run with hit lines. Every result carries the lines of its matches, the renderers read those (the
    // text of a gz pack stays on the device), and "Lines with matches" is the device's count as with line context.
    bool gather = false;
    // --gz-members: gz packs hold files of one member or many (matchy_multi_scanner_submit_gz_files); the verdicts are per file
    bool gz_members = false;
    // --render-on-gpu: a batch whose line bases are known when it is submitted leaves the device as finished NDJSON
    // (matchy_multi_scanner_set_render): every batch without line numbers; with them the packs (every segment is a whole file: base 0)
    // and an input's first batch. Any other batch, and a batch whose render status is not OK, goes through the host renderer as before.
    bool render_gpu = false;
    std::vector<char> input_started;   // the reader's: the input has had a batch submitted
    std::atomic<size_t> gpu_batches{0}, gpu_fallback{0};
    std::atomic<unsigned long long> gpu_bytes{0};
    // --whole-lines: the scanners' counters of every batch (queries, address, string, invalid UTF-8), summed for -s
    bool whole_lines = false;
    std::atomic<unsigned long long> wl_counters[4] = {{0}, {0}, {0}, {0}};
    void add_whole_lines(const matchy_scanner_t* sc) {
        uint64_t c[4] = {0, 0, 0, 0};
        matchy_scanner_get_whole_lines_counters(sc, c);
        for (int k = 0; k < 4; ++k) wl_counters[k] += c[k];
    }
    std::vector<unsigned long long> line_base;   // per input; the printer's (then --follow's)
    // arms the library for the batch about to be submitted, where its line bases are known
    void arm(Batch& b) {
        if (!render_gpu || !json) return;
        const bool segmented = !b.pack.empty() || !b.gz.empty();
        bool first = true;
        if (!segmented || b.window) {   // a window is a batch of its input like a stream batch: only the first has line base 0
            if (input_started.size() <= b.input) input_started.resize(b.input + 1, 0);
            first = !input_started[b.input];
            input_started[b.input] = 1;
        }
        if (line_ctx && (!segmented || b.window) && !first) return;
        matchy_render_params_t p;
        memset(&p, 0, sizeof(p));
        p.flags = line_ctx ? (MATCHY_RENDER_LINE_NUMBERS | (input_line ? MATCHY_RENDER_INPUT_LINE : 0u)) : 0u;
        std::vector<const char*> src;
        if (segmented) { src = pack_sources(b); p.sources = src.data(); p.n_sources = src.size(); }
        else p.source = sources[b.input].c_str();
        b.armed = matchy_multi_scanner_set_render(ms, &p) == MATCHY_SUCCESS;   // copied at the call
    }
    // the block of an armed batch as the text of its Done; false: not rendered there (the host renderer takes over)
    bool take_gpu_text(const matchy_scan_result_t& r, Done& d) {
        const char* text = nullptr;
        uint64_t n = 0;
        int32_t status = MATCHY_RENDER_OK;
        if (matchy_scan_result_ndjson(&r, &text, &n, &status) != MATCHY_SUCCESS || status != MATCHY_RENDER_OK) { ++gpu_fallback; return false; }
        if (n) {
            char* copy = (char*)malloc(n);   // the result goes when the hook returns; the printer frees this like the host renderer's buffer
            if (!copy) { ++gpu_fallback; return false; }
            memcpy(copy, text, n);
            d.text = copy; d.text_len = n;
        }
        ++gpu_batches; gpu_bytes += n;
        return true;
    }

    // every input a batch carries: its own, or the files of a pack
    template <class F> static void each_input(const Batch& b, F&& f) {
        if (!b.gz.empty()) for (const GzFile& g : b.gz) f(g.input);
        else if (b.pack.empty()) f(b.input);
        else for (const PackedInput& pi : b.pack) f(pi.input);
    }
    // the batch goes to the library's queue; its Batch object travels as the tag and comes back with the result
    size_t submit(Batch&& b) {
        Batch* hb = new Batch(std::move(b));
        size_t seq;
        { std::lock_guard<std::mutex> lk(mu); seq = submitted++; }
        int32_t rc;
        arm(*hb);
        if (!hb->gz.empty()) {   // the text comes back only where something is rendered from it
            if (hb->window) {
                const matchy_gz_window_t w{hb->carry.data(), (uint32_t)hb->carry.size(), hb->carry_cap, hb->window_last ? MATCHY_WINDOW_LAST : 0u};
                rc = matchy_multi_scanner_submit_gz_window(ms, hb->ptr, hb->len, &w, json && !gather && !hb->armed, hb);
            } else if (gz_members) {
                std::vector<matchy_gz_file_t> table;
                for (const GzFile& g : hb->gz) table.push_back(matchy_gz_file_t{g.offset, g.len});
                rc = matchy_multi_scanner_submit_gz_files(ms, hb->ptr, hb->len, table.data(), table.size(), json && !gather && !hb->armed, hb);
            } else {
                std::vector<matchy_gz_member_t> table;
                for (const GzFile& g : hb->gz) table.push_back(matchy_gz_member_t{g.offset, g.len, 0});
                rc = matchy_multi_scanner_submit_gz(ms, hb->ptr, hb->len, table.data(), table.size(), json && !gather && !hb->armed, hb);
            }
            if (rc != MATCHY_SUCCESS) { matchy_multi_scanner_set_render(ms, nullptr); hb->verdict->set(nullptr, 0); delete hb; return seq; }   // every member goes the old way
        }
        else if (hb->pack.empty()) rc = matchy_multi_scanner_submit(ms, hb->ptr, hb->len, hb, hb->reg);
        else {
            std::vector<uint32_t> starts;
            for (const PackedInput& pi : hb->pack) starts.push_back(pi.start);
            rc = matchy_multi_scanner_submit_segments(ms, hb->ptr, hb->len, starts.data(), starts.size(), hb, hb->reg);
        }
        if (rc != MATCHY_SUCCESS) {
            matchy_multi_scanner_set_render(ms, nullptr);   // the parameters go with a batch that was queued, never with the next one
            // not queued (cannot happen for batches below 4 GiB): the printer never sees it
            fprintf(stderr, "[ERROR] batch of %zu bytes rejected: %s\n", hb->len, matchy_amd_last_error());
            { std::lock_guard<std::mutex> lk(mu); each_input(*hb, [&](size_t i) { rejected_inputs.push_back(i); }); }   // its matches are missing: the inputs count as failed
            if (hb->reg) matchy_amd_host_unregister(hb->reg);
            delete hb;
        }
        return seq;
    }
    // Mapped inputs: the mapping of a file is released by the printer as soon as the file's last batch has been printed — the
    // page tables of a file of gigabytes take tens of milliseconds to tear down, and that runs beside the scans of the next
    // files instead of behind the last one.
    // bytes of each input the first pass has read: where --follow starts watching (a size taken AFTER that pass would skip what was appended in between)
    std::vector<long long> consumed;
    std::vector<size_t> rejected_inputs;   // guarded by mu: inputs with a batch the library did not take
    struct Mapping { void* p; size_t len; size_t last_seq; bool released; };
    std::vector<Mapping> mappings;   // guarded by mu
    void add_mapping(void* p, size_t len, size_t last_seq) { std::lock_guard<std::mutex> lk(mu); mappings.push_back({p, len, last_seq, false}); }
    void release_mappings(size_t printed_below) {   // every batch with seq < printed_below is done
        std::vector<Mapping> go;
        {
            std::lock_guard<std::mutex> lk(mu);
            for (Mapping& m : mappings) if (!m.released && m.last_seq < printed_below) { m.released = true; go.push_back(m); }
        }
        for (const Mapping& m : go) munmap(m.p, m.len);
    }
    // what one batch contributes to the output: counters, and (json) its matches rendered — on the worker thread that scanned it
    void render(matchy_scanner_t* sc, const matchy_scan_result_t& r, const uint8_t* data, size_t len, const Batch& b, Done& d) {
        const size_t input = b.input;
        d.input = input;
        Totals& t = d.t;
        const bool segmented = !b.pack.empty() || !b.gz.empty();
        if (!b.gz.empty() && b.armed && data == nullptr) {
            // an armed gz pack came without its text: where its block is not to be had nothing can be rendered from it, and every
            // member is read the old way, as if the GPU had accepted none
            int32_t status = MATCHY_RENDER_OK;
            if (matchy_scan_result_ndjson(&r, nullptr, nullptr, &status) != MATCHY_SUCCESS || status != MATCHY_RENDER_OK) { ++gpu_fallback; d.skip = true; b.verdict->set(nullptr, 0); return; }
        }
        if (!b.gz.empty()) {
            // a gz pack: lines and bytes are those of the members the GPU accepted (separators and the regions of the others are not
            // counted); the others are read the old way by the reader, which waits for this verdict
            t.lines += r.lines; t.candidates += r.candidates; t.bytes += r.bytes; t.matches += r.n_hits;
            const int32_t* st = nullptr;
            size_t n_st = 0;
            const int32_t got = gz_members ? matchy_scan_result_gz_files(&r, &st, &n_st, nullptr) : matchy_scan_result_gz(&r, &st, &n_st, nullptr, nullptr);   // per file either way
            if (got != MATCHY_SUCCESS) { st = nullptr; n_st = 0; d.ok = false; }
            if (b.window && got == MATCHY_SUCCESS) {
                const uint8_t* carry = nullptr;
                size_t n_carry = 0;
                if (matchy_scan_result_gz_window(&r, &b.verdict->window_status, &carry, &n_carry) == MATCHY_SUCCESS) { b.verdict->carry.assign(carry, carry + n_carry); b.verdict->bytes = r.bytes; }
                else { st = nullptr; n_st = 0; d.ok = false; }
            }
            b.verdict->set(st, n_st);
            if (!d.ok) { fprintf(stderr, "[ERROR] no gz statuses in the scan result of a gz pack: %s\n", matchy_amd_last_error()); return; }
        } else {
            // a pack: the newlines the packer appended are not the inputs'
            t.lines += r.lines - b.appended; t.candidates += r.candidates; t.bytes += len - b.appended; t.matches += r.n_hits;
        }
        // an armed gz pack comes back without its text: the library scans it with line context, and its "Lines with matches" are the
        // table's like those of any pack scanned with line context (plain batches of the same run are counted from their text as before)
        const bool table_counts = line_ctx || gather || (b.armed && !b.gz.empty());
        if (table_counts && segmented) {   // per segment, from the table the GPU filled
            const matchy_scan_segment_t* segs = nullptr;
            size_t n_segs = 0;
            if (matchy_scan_result_segments(&r, nullptr, nullptr, &segs, &n_segs) == MATCHY_SUCCESS) for (size_t k = 0; k < n_segs; ++k) t.lines_with_matches += segs[k].lines_with_matches;
            else { fprintf(stderr, "[ERROR] no segments in the scan result of a pack: %s\n", matchy_amd_last_error()); d.ok = false; }
            if (line_ctx || !d.ok) return;
        } else if (line_ctx || gather) {
            uint64_t lwm = 0;
            if (matchy_scan_result_lines(&r, nullptr, nullptr, &lwm) == MATCHY_SUCCESS) t.lines_with_matches += lwm;
            else { fprintf(stderr, "[ERROR] no line context in a scan result: %s\n", matchy_amd_last_error()); d.ok = false; }
            if (line_ctx || !d.ok) return;   // the records of a scan with line numbers: render_numbered, in sequence order
        } else {
            // lines with matches: hits come sorted by offset; a new line starts when a '\n' lies between two hit starts (and a '\n' lies
            // between any two segments of a pack)
            size_t prev = (size_t)-1;
            for (size_t i = 0; i < r.n_hits; ++i) {
                const size_t s = (size_t)r.hits[i].start;
                if (prev == (size_t)-1 || memchr(data + prev, '\n', s - prev)) ++t.lines_with_matches;
                prev = s;
            }
        }
        const std::string& source = sources[input];
        if (json && r.n_hits && b.armed && take_gpu_text(r, d)) return;
        if (json && r.n_hits) {   // every match of the batch in one call (the scanner caches the rendered data payloads)
            char* text = nullptr;
            size_t n = 0;
            int32_t rc;
            if (!segmented) rc = matchy_scan_result_to_ndjson(sc, &r, data, source.c_str(), &text, &n);
            else { const std::vector<const char*> src = pack_sources(b); rc = matchy_scan_result_to_ndjson_segments(sc, &r, data, src.data(), nullptr, false, &text, &n); }
            if (rc == MATCHY_SUCCESS) { d.text = text; d.text_len = n; }
            else { fprintf(stderr, "[ERROR] rendering failed: %s\n", matchy_amd_last_error()); d.ok = false; }
        }
    }
    std::vector<const char*> pack_sources(const Batch& b) const {
        std::vector<const char*> src;
        for (const PackedInput& pi : b.pack) src.push_back(sources[pi.input].c_str());
        for (const GzFile& g : b.gz) src.push_back(sources[g.input].c_str());
        return src;
    }
    // the records of a batch of a scan with line context; `base` = lines of its input in front of it
    // (a packed input is whole: its lines count from zero)
    void render_numbered(matchy_scanner_t* sc, const matchy_scan_result_t& r, const uint8_t* data, const Batch& b, unsigned long long base, Done& d) {
        if (!json || !r.n_hits || !d.ok || d.skip) return;
        if (b.armed && take_gpu_text(r, d)) return;   // armed batches have base 0: a pack, or an input's first batch
        char* text = nullptr;
        size_t n = 0;
        int32_t rc;
        if (b.pack.empty() && b.gz.empty()) rc = matchy_scan_result_to_ndjson_lines(sc, &r, data, sources[b.input].c_str(), base, input_line, &text, &n);
        else {
            const std::vector<const char*> src = pack_sources(b);
            const std::vector<uint64_t> bases(src.size(), b.window ? base : 0);   // a window goes on where the windows in front ended
            rc = matchy_scan_result_to_ndjson_segments(sc, &r, data, src.data(), bases.data(), input_line, &text, &n);
        }
        if (rc == MATCHY_SUCCESS) { d.text = text; d.text_len = n; }
        else { fprintf(stderr, "[ERROR] rendering failed: %s\n", matchy_amd_last_error()); d.ok = false; }
    }
    static void* batch_hook(void* user, size_t, matchy_scanner_t* sc, const matchy_scan_result_t* r, const uint8_t* data, size_t len, void* tag) {
        MatchPipeline* pl = (MatchPipeline*)user;
        Done* d = new Done();
        if (pl->whole_lines) pl->add_whole_lines(sc);
        pl->render(sc, *r, data, len, *(const Batch*)tag, *d);
        return d;
    }
    // scan one batch on the calling thread and render its matches (--follow: one scanner, batches as they appear)
    void run_batch(matchy_scanner_t* sc, Batch& b, Done& d) {
        d.input = b.input;
        if (!b.len) return;
        matchy_scan_result_t r;
        memset(&r, 0, sizeof(r));
        if (matchy_scanner_scan(sc, b.ptr, b.len, &r) != MATCHY_SUCCESS) {
            fprintf(stderr, "[ERROR] scan failed: %s\n", matchy_amd_last_error());
            d.ok = false;
            return;
        }
        if (whole_lines) add_whole_lines(sc);
        render(sc, r, b.ptr, b.len, b, d);
        if (line_ctx) {   // --follow: batches of an input come one after the other, the count continues across the polls
            render_numbered(sc, r, b.ptr, b, line_base[b.input], d);
            line_base[b.input] += r.lines;
        }
        matchy_scan_result_free(&r);
    }
    // takes the batches back in sequence order and prints them, until the reader is done and nothing is pending
    void printer(Totals& total, std::vector<char>& input_failed) {
        for (;;) {
            matchy_multi_batch_t b;
            int32_t r = matchy_multi_scanner_next(ms, &b);
            if (r == 0) {
                if (!reader_done) { std::this_thread::sleep_for(std::chrono::microseconds(200)); continue; }   // between two submits
                r = matchy_multi_scanner_next(ms, &b);
                if (r == 0) return;
            }
            if (r != 1) { fprintf(stderr, "[ERROR] gathering results failed: %s\n", matchy_amd_last_error()); return; }
            Batch* hb = (Batch*)b.tag;
            Done* d = (Done*)b.payload;
            if (b.status != MATCHY_SUCCESS) {
                if (!hb->gz.empty()) hb->verdict->set(nullptr, 0);   // the pack was not scanned: the reader reads its files the old way
                else {
                    fprintf(stderr, "[ERROR] scan failed: %s\n", matchy_amd_last_error());
                    each_input(*hb, [&](size_t i) { input_failed[i] = 1; });
                }
            } else if (d) {
                if (line_ctx) {   // the worker's scanner renders here: with line context its hook renders nothing, so one thread at a time uses it
                    render_numbered(matchy_multi_scanner_worker_scanner(ms, b.worker), b.result, b.data, *hb, line_base[hb->input], *d);
                    if ((hb->pack.empty() && hb->gz.empty()) || hb->window) line_base[hb->input] += b.result.lines;
                }
                if (!d->ok) each_input(*hb, [&](size_t i) { input_failed[i] = 1; });   // rendering failed: the batch's matches are missing, exit status says so
                if (d->text_len) write_all_stdout(d->text, d->text_len);
                total.lines += d->t.lines; total.lines_with_matches += d->t.lines_with_matches; total.matches += d->t.matches;
                total.candidates += d->t.candidates; total.bytes += d->t.bytes;
            }
            matchy_scan_result_free(&b.result);
            delete d;
            delete hb;   // frees an owned (read) batch's bytes; a mapped batch's pages go with its file's mapping
            release_mappings(b.seq + 1);
        }
    }
};

// Inputs ending in .gz (case-insensitive) are decompressed on the fly like the reference's file reader does
// (crates/matchy/src/file_reader.rs:45-75, by extension); "-" is stdin. Regular files are mapped and their batches are
// views of the mapping (no copy on the host; this thread pre-faults and pins each batch's pages ahead of its scan;
// MATCHY_AMD_NO_MMAP=1 reads them like a stream instead). Returns false when the input could not be read. Mappings are
// released by the printer as their files complete. skip (inputs that are read): the first `skip` bytes of the stream — what the gz windows
// in front have reported already (--gz-windows), which ends behind a '\n' — are read and cut into batches like the rest, so the cuts
// are those of the whole stream, but not submitted; 0 is the whole input.
bool read_input(MatchPipeline& pl, size_t input, const std::string& path, size_t batch_bytes, uint64_t skip = 0) {
    const bool gz = ends_with_ci(path, ".gz");
    int fd = path == "-" ? 0 : open(path.c_str(), O_RDONLY);
    if (fd < 0) { fprintf(stderr, "[ERROR] Failed to process %s: %s\n", path.c_str(), strerror(errno)); return false; }
    struct stat sb;
    if (!gz && fd != 0 && fstat(fd, &sb) == 0 && S_ISREG(sb.st_mode) && sb.st_size > 0 && !getenv("MATCHY_AMD_NO_MMAP")) {
        const size_t size = (size_t)sb.st_size;
        void* m = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
        if (m != MAP_FAILED) {
            close(fd);
            (void)madvise(m, size, MADV_SEQUENTIAL);
            const uint8_t* base = (const uint8_t*)m;
            size_t last_seq = 0;
            for (size_t pos = 0; pos < size;) {
                const size_t end = newline_cut(base, pos, size, batch_bytes);
                Batch b;
                b.input = input; b.ptr = base + pos; b.len = end - pos; b.mapped = true;
                b.reg = prefault_and_pin(b.ptr, b.len);
                last_seq = pl.submit(std::move(b));
                pos = end;
            }
            pl.add_mapping(m, size, last_seq);
            if (input < pl.consumed.size()) pl.consumed[input] = (long long)size;
            return true;
        }
    }
    gzFile zf = nullptr;
    if (gz) {
        zf = gzdopen(fd, "rb");
        if (!zf) { fprintf(stderr, "[ERROR] Failed to process %s: cannot start gzip decoder\n", path.c_str()); close(fd); return false; }
        gzbuffer(zf, 1u << 20);
    }
    size_t total_read = 0;
    const StreamEnd e = read_batches(
        [&](void* p, size_t n) {
            const ssize_t r = gz ? (ssize_t)gzread(zf, p, (unsigned)n) : read(fd, p, n);
            if (r < 0 && gz) errno = EIO;   // the decoder keeps its error: a retry would fail again
            return r;
        },
        batch_bytes,
        [&](Bytes&& data, size_t len, uint64_t off) {
            total_read += len;
            if (off + len <= skip) return true;   // reported already
            const size_t drop = off < skip ? (size_t)(skip - off) : 0;   // skip lies behind a '\n': what is left starts a line
            Batch b;
            b.input = input; b.ptr = data.get() + drop; b.len = len - drop; b.own = std::move(data);
            pl.submit(std::move(b));
            return true;
        });
    const bool ok = e == StreamEnd::DONE;
    if (!ok) { int ze; fprintf(stderr, "[ERROR] Failed to process %s: %s\n", path.c_str(), gz && errno == EIO ? gzerror(zf, &ze) : strerror(errno)); }
    if (gz) gzclose(zf);   // closes fd as well
    else if (fd) close(fd);
    if (ok && !gz && fd != 0 && input < pl.consumed.size()) pl.consumed[input] = (long long)total_read;
    return ok;
}

// -f / --follow (match_processor/follow.rs:20-264): after the existing content, keep watching the files and scan what is
// appended — from the last known size to the new one, whatever it ends with, as the reference's `reader.lines()` does; a
// file that shrank is read again from the start; a file that disappeared is reported once. Records carry the wall-clock
// time of their batch as `timestamp` (the parallel path's constant "0.000" everywhere else). Ends on SIGINT / SIGTERM.
volatile sig_atomic_t g_stop = 0;
void on_stop(int) { g_stop = 1; }

void follow_inputs(MatchPipeline& pl, matchy_scanner_t* sc, const std::vector<std::string>& paths, bool stats, Totals& total) {
    struct Tail { std::string path; size_t input; off_t pos; bool gone; };
    std::vector<Tail> tails;
    for (size_t i = 0; i < paths.size(); ++i) {
        struct stat sb;
        // from where the first pass stopped reading; inputs it could not count (.gz, unreadable): from their size now
        const bool counted = i < pl.consumed.size() && pl.consumed[i] >= 0;
        tails.push_back({paths[i], i, counted ? (off_t)pl.consumed[i] : (stat(paths[i].c_str(), &sb) == 0 ? sb.st_size : 0), false});
    }
    struct sigaction sa;
    memset(&sa, 0, sizeof(sa));
    sa.sa_handler = on_stop;
    sigaction(SIGINT, &sa, nullptr);
    sigaction(SIGTERM, &sa, nullptr);
    if (stats) fprintf(stderr, "[INFO] Watching for new content (Ctrl+C to stop)...\n");
    while (!g_stop) {
        bool any = false;
        for (Tail& tl : tails) {
            struct stat sb;
            if (stat(tl.path.c_str(), &sb) != 0) {
                if (!tl.gone && stats) fprintf(stderr, "[WARN] File deleted/rotated: %s\n", tl.path.c_str());
                tl.gone = true;
                continue;
            }
            tl.gone = false;
            if (sb.st_size < tl.pos) { tl.pos = 0; if (tl.input < pl.line_base.size()) pl.line_base[tl.input] = 0; }   // truncated: start over
            if (sb.st_size == tl.pos) continue;
            const int fd = open(tl.path.c_str(), O_RDONLY);
            if (fd < 0) continue;
            Batch b;
            b.input = tl.input;
            b.own.reset((uint8_t*)malloc((size_t)(sb.st_size - tl.pos) + 16));
            if (!b.own) { close(fd); continue; }
            size_t have = 0;
            while (have < (size_t)(sb.st_size - tl.pos)) {
                const ssize_t n = pread(fd, b.own.get() + have, (size_t)(sb.st_size - tl.pos) - have, tl.pos + (off_t)have);
                if (n <= 0) break;
                have += (size_t)n;
            }
            close(fd);
            tl.pos += (off_t)have;
            if (!have) continue;
            any = true;
            b.ptr = b.own.get(); b.len = have;
            Done d;
            pl.run_batch(sc, b, d);
            if (d.text_len) d.out.assign(d.text, d.text_len);
            if (!d.out.empty()) {
                // this batch's records carry the current time
                char ts[48];
                struct timespec now;
                clock_gettime(CLOCK_REALTIME, &now);
                snprintf(ts, sizeof(ts), "\"timestamp\":\"%.3f\"}", (double)now.tv_sec + (double)now.tv_nsec * 1e-9);
                static const std::string fixed = "\"timestamp\":\"0.000\"}";
                std::string out;
                size_t from = 0;
                for (;;) {
                    const size_t k = d.out.find(fixed + "\n", from);
                    if (k == std::string::npos) { out.append(d.out, from, std::string::npos); break; }
                    out.append(d.out, from, k - from);
                    out += ts;
                    from = k + fixed.size();
                }
                fwrite(out.data(), 1, out.size(), stdout);
                fflush(stdout);
            }
            total.lines += d.t.lines; total.lines_with_matches += d.t.lines_with_matches; total.matches += d.t.matches;
            total.candidates += d.t.candidates; total.bytes += d.t.bytes;
        }
        if (!any) usleep(100 * 1000);
    }
    if (stats) fprintf(stderr, "[INFO] Follow mode stopped\n");
}

// --gz-on-gpu, the reader's side. take(i) reads an eligible .gz input — a regular file of at least 18 bytes whose header parses, compressed
// size and ISIZE both at most batch_bytes / 4 (MATCHY_AMD_GZ_MAX_MEMBER lowers that) — into the pack in hand; a pack holds up to batch_bytes
// of inflated text and goes out when the next file would pass that. Before anything else is submitted, barrier() sends the pack in
// hand and waits for the verdict on it: the members the GPU did not accept are read the old way there, right behind their pack, so
// the order of everything else is that of the command line. While a pack is on the GPU the reader goes on reading files for the next.
struct GzPacker {
    MatchPipeline& pl;
    const std::vector<std::string>& paths;
    std::vector<char>& read_failed;
    size_t batch_bytes, max_member;
    std::vector<uint8_t> buf;          // the files of the pack in hand, compressed, end to end
    std::vector<GzFile> files;
    uint64_t text = 0;                 // inflated bytes of the pack in hand, separators included
    std::shared_ptr<GzVerdict> pending;
    std::vector<GzFile> pending_files;
    size_t on_gpu = 0, packs = 0, on_host = 0;
    unsigned long long packed_bytes = 0, text_bytes = 0;
    // --gz-members: a .gz input of many members is eligible when every member's compressed length and ISIZE are at most max_member and the
    // file, compressed and inflated (the sum of its ISIZEs plus 1), fits one pack; the verdict on the pack is then per file
    bool members = false;
    std::vector<uint64_t> cuts;
    size_t multi_files = 0, multi_members = 0;   // of the files the GPU accepted: those of more than one member, and their members

    // --gz-windows: a multi-member .gz input that take() leaves (larger than a batch, or more text than a pack holds) is mapped and goes
    // out as a chain of windows of whole members: up to batch_bytes - carry_cap of text and batch_bytes compressed each. carry_cap is
    // min(1 MiB, max_member); MATCHY_AMD_GZ_MAX_CARRY lowers it.
    bool windows = false;
    size_t carry_cap = 0;
    size_t win_windows = 0, win_files = 0, win_host = 0;   // windows the GPU accepted, files that went out as windows, of those finished on the host

    GzPacker(MatchPipeline& p, const std::vector<std::string>& ps, std::vector<char>& rf, size_t bb) : pl(p), paths(ps), read_failed(rf) {
        batch_bytes = std::min<size_t>(bb, ((size_t)1 << 31) - ((size_t)1 << 20));   // a batch stays below 2^31 bytes
        max_member = batch_bytes / 4;
        if (const char* e = getenv("MATCHY_AMD_GZ_MAX_MEMBER")) max_member = std::min<size_t>(max_member, strtoull(e, nullptr, 10));
        carry_cap = std::min<size_t>((size_t)1 << 20, max_member);
        if (const char* e = getenv("MATCHY_AMD_GZ_MAX_CARRY")) carry_cap = std::min<size_t>(carry_cap, strtoull(e, nullptr, 10));
    }
    // --gz-windows, behind barrier(): input i as a chain of windows. False: not eligible (no regular .gz file, a first header that does
    // not parse, a first member that alone breaks a bound), nothing was submitted and the input is read the way it is without the flag.
    // The windows go out one at a time: the reader waits for a window's verdict, and with it the carry, before it submits the next —
    // and faults the next window's pages in meanwhile. A window the GPU does not accept (a member that fails, NO_LINE_END, a scan that
    // failed) or a member the walker cannot take ends the chain: everything reported so far is right — verified members, complete
    // lines only — and the host reads the file the way it does without the flag and reports what lies behind the bytes the accepted
    // windows consumed. A file whose decoder fails loses the batch the host was filling, as it does without the flag: the records are
    // those of the run without the flag, plus — where the windows had got further than the host's last batch cut — the complete lines
    // in between.
    bool take_windows(size_t i) {
        const std::string& path = paths[i];
        struct stat sb;
        if (!windows || !pack_ends_with_gz(path)) return false;
        const int fd = open(path.c_str(), O_RDONLY);
        if (fd < 0) return false;
        if (fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode) || sb.st_size < 18) { close(fd); return false; }
        const size_t size = (size_t)sb.st_size;
        void* m = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
        close(fd);
        if (m == MAP_FAILED) return false;
        const uint8_t* p = (const uint8_t*)m;
        const uint64_t max_text = batch_bytes - carry_cap;   // carry_cap <= max_member = batch_bytes / 4
        GzWindow cur, nxt;
        if (!gz_next_window(p, size, 0, batch_bytes, max_text, max_member, cur)) { munmap(m, size); return false; }
        ++win_files;
        std::vector<uint8_t> carry;
        uint64_t from = 0, consumed = 0;
        size_t last_seq = 0;
        bool ok = false;
        for (;;) {
            Batch b;
            b.input = i; b.ptr = p + from; b.len = (size_t)(cur.end - from); b.mapped = true;
            b.window = true; b.window_last = cur.end == size; b.carry = carry; b.carry_cap = (uint32_t)carry_cap;
            b.gz.push_back(GzFile{i, 0, (uint32_t)b.len, (uint32_t)cur.text, cur.members});
            b.verdict = std::make_shared<GzVerdict>();
            const std::shared_ptr<GzVerdict> v = b.verdict;
            last_seq = pl.submit(std::move(b));
            const bool have_next = cur.end < size && gz_next_window(p, size, cur.end, batch_bytes, max_text, max_member, nxt);
            if (have_next) { volatile uint8_t sink = 0; for (uint64_t q = cur.end; q < nxt.end; q += 4096) sink = sink + p[q]; }
            v->wait();
            if (v->status.size() != 1 || v->status[0] != MATCHY_GZ_OK || v->window_status != MATCHY_WINDOW_OK) break;
            ++win_windows; consumed += v->bytes;
            carry = std::move(v->carry);
            if (cur.end == size) { ok = true; break; }
            if (!have_next) break;   // the next member alone breaks a bound
            from = cur.end; cur = nxt;
        }
        pl.add_mapping(m, size, last_seq);
        if (!ok) { ++win_host; if (!read_input(pl, i, path, batch_bytes, consumed)) read_failed[i] = 1; }
        return true;
    }
    // --gz-members: the members of the file p[0, size), whose first header parses. False: a member's compressed length or ISIZE above
    // max_member, a piece with no room for its trailer, or more text than one pack holds — the file keeps the host path.
    bool members_fit(const uint8_t* p, size_t size, uint32_t& n_members, uint32_t& isize) {
        gz_split_members(p, size, cuts);
        uint64_t sum = 0;
        for (size_t k = 0; k < cuts.size(); ++k) {
            const uint64_t at = cuts[k], len = (k + 1 < cuts.size() ? cuts[k + 1] : (uint64_t)size) - at;
            uint64_t body = 0;
            if (len > max_member || gz_parse_header(p + at, len, body) != GZ_PLAN_OK || len - body < 8) return false;
            const uint8_t* t = p + at + len - 4;
            const uint32_t is = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
            if (is > max_member) return false;
            sum += is;
            if (sum + 1 > batch_bytes) return false;
        }
        n_members = (uint32_t)cuts.size(); isize = (uint32_t)sum;
        return true;
    }
    bool take(size_t i) {
        const std::string& path = paths[i];
        struct stat sb;
        // with --gz-members a file may be as large as a pack: its members are what must be small
        if (!pack_ends_with_gz(path) || stat(path.c_str(), &sb) != 0 || !S_ISREG(sb.st_mode) || sb.st_size < 18 || (size_t)sb.st_size > (members ? batch_bytes : max_member)) return false;
        const size_t size = (size_t)sb.st_size, at = buf.size();
        buf.resize(at + size);
        uint64_t body = 0;
        const bool whole = pack_read_file(path, buf.data() + at, size) == (long long)size;
        const bool parses = whole && gz_parse_header(buf.data() + at, size, body) == GZ_PLAN_OK && size - body >= 8;
        const uint8_t* t = buf.data() + at + size - 4;
        uint32_t isize = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24, n_members = 1;
        if (parses && members && !members_fit(buf.data() + at, size, n_members, isize)) { buf.resize(at); return false; }
        // a file of one member is treated as it is without --gz-members
        if (!parses || (n_members == 1 && (size > max_member || isize > max_member))) { buf.resize(at); return false; }
        // the file opens the next pack: its text does not fit, or (--gz-members, where a file of many empty members may be as large as a
        // pack and vouch for no text) its compressed bytes do not
        if (!files.empty() && (text + isize + 1 > batch_bytes || (members && at + size > batch_bytes))) {
            const std::vector<uint8_t> file(buf.begin() + (long)at, buf.end());
            buf.resize(at);
            flush();
            buf = file;
        }
        files.push_back(GzFile{i, buf.size() - size, (uint32_t)size, isize, n_members});
        text += (uint64_t)isize + 1;
        return true;
    }
    // the verdict on the pack that is out: what the GPU accepted is counted, the rest is read the old way now
    void settle() {
        if (!pending) return;
        pending->wait();
        for (size_t k = 0; k < pending_files.size(); ++k) {
            const GzFile& g = pending_files[k];
            if (k < pending->status.size() && pending->status[k] == MATCHY_GZ_OK) {
                ++on_gpu; packed_bytes += g.len; text_bytes += g.isize;
                if (g.members > 1) { ++multi_files; multi_members += g.members; }
                continue;
            }
            ++on_host;
            if (!read_input(pl, g.input, paths[g.input], batch_bytes)) read_failed[g.input] = 1;
        }
        pending.reset();
        pending_files.clear();
    }
    void flush() {
        settle();
        if (files.empty()) return;
        Batch b;
        b.own.reset((uint8_t*)malloc(buf.size()));
        if (!b.own) {   // no memory for the pack: its files go the old way
            for (const GzFile& g : files) { ++on_host; if (!read_input(pl, g.input, paths[g.input], batch_bytes)) read_failed[g.input] = 1; }
        } else {
            memcpy(b.own.get(), buf.data(), buf.size());
            b.input = files[0].input; b.ptr = b.own.get(); b.len = buf.size();
            b.gz = files; b.verdict = std::make_shared<GzVerdict>();
            pending = b.verdict; pending_files = files;
            ++packs;
            pl.submit(std::move(b));
        }
        buf.clear(); files.clear(); text = 0;
    }
    void barrier() { flush(); settle(); }
};

int cmd_match(int argc, char** argv) {
    std::vector<std::string> pos;
    std::string format = "json", extractors, devices;
    bool stats = false, follow = false, line_numbers = false, input_line = false, tally = false, pack = false, gz_gpu = false, gz_members = false, gz_windows = false, gather_lines = false, render_gpu = false, whole_lines = false;
    size_t tally_limit = 20;   // --tally[=N]: rows of the report, 0 = all
    size_t batch_bytes = (size_t)256 << 20;  // GPU batches: large, so that one launch amortises PCIe latency
    int device = 0;
    int jobs = 0;   // -j N|auto (matchy.rs:98-103: worker threads): scanners here; auto = 2 (summary) / 4 (json) per device listed once
    if (const char* d = getenv("MATCHY_AMD_DEVICE")) device = atoi(d);
    for (int i = 0; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&](const char* name) -> const char* { if (i + 1 >= argc) { fprintf(stderr, "error: %s needs a value\n", name); exit(2); } return argv[++i]; };
        auto eqval = [&](const char* name, std::string& out) {  // --name=value or --name value
            size_t n = strlen(name);
            if (a.compare(0, n, name) != 0) return false;
            if (a.size() == n) { out = next(name); return true; }
            if (a[n] == '=') { out = a.substr(n + 1); return true; }
            return false;
        };
        std::string v;
        if (eqval("--format", v)) format = v;
        else if (a == "-s" || a == "--stats") stats = true;
        else if (eqval("--batch-bytes", v)) { size_t b = strtoull(v.c_str(), nullptr, 10); if (b >= 4096) batch_bytes = b; }
        else if (eqval("--extractors", v)) extractors = v;
        else if (eqval("--devices", v)) devices = v;
        else if (eqval("--device", v)) device = atoi(v.c_str());
        else if (eqval("--threads", v) || eqval("--readers", v) || eqval("--cache-size", v)) {}
        else if (a == "-j") { const std::string j = next("-j"); jobs = j == "auto" ? 0 : std::max(0, atoi(j.c_str())); }
        else if (a == "-p" || a == "--progress" || a == "--debug-routing") {}
        else if (a == "-f" || a == "--follow") follow = true;
        else if (a == "--line-numbers") line_numbers = true;
        else if (a == "--input-line") input_line = true;
        else if (a == "--pack-inputs") pack = true;
        else if (a == "--gz-on-gpu") gz_gpu = true;
        else if (a == "--gz-members") gz_members = true;
        else if (a == "--gz-windows") gz_windows = true;
        else if (a == "--gather-lines") gather_lines = true;
        else if (a == "--render-on-gpu") render_gpu = true;
        else if (a == "--whole-lines") whole_lines = true;
        else if (a == "--tally") tally = true;
        else if (a.compare(0, 8, "--tally=") == 0) {
            const std::string n = a.substr(8);
            if (n.empty() || n.find_first_not_of("0123456789") != std::string::npos) { fprintf(stderr, "error: --tally=N needs a number, got '%s'\n", n.c_str()); return 2; }
            tally = true; tally_limit = strtoull(n.c_str(), nullptr, 10);
        }
        else if (a.size() > 1 && a[0] == '-') { fprintf(stderr, "error: unexpected argument '%s'\n", a.c_str()); return 2; }
        else pos.push_back(a);
    }
    if (pos.size() < 2) return usage();
    if (format != "json" && format != "summary") { fprintf(stderr, "Error: Unknown format: %s. Use 'json' or 'summary'\n", format.c_str()); return 1; }
    if (gz_windows && !(gz_gpu && gz_members)) { fprintf(stderr, "Error: --gz-windows needs --gz-on-gpu --gz-members (it extends them to multi-member files larger than a batch)\n"); return 1; }
    if (gz_members && !gz_gpu) { fprintf(stderr, "Error: --gz-members needs --gz-on-gpu (it extends the gz packs to files of many members)\n"); return 1; }
    if (whole_lines) {
        // the mode has no extraction to configure, and the library refuses it together with segments, gz scans, hit lines and rendered records
        const char* other = !extractors.empty() ? "--extractors" : pack ? "--pack-inputs" : gz_gpu ? "--gz-on-gpu" : gather_lines ? "--gather-lines" : render_gpu ? "--render-on-gpu" : nullptr;
        if (other) { fprintf(stderr, "Error: --whole-lines is not supported with %s\n", other); return 1; }
    }
    if (follow && tally) { fprintf(stderr, "Error: --tally is not supported with --follow (the report is printed after the last batch)\n"); return 1; }
    if (follow && pack) { fprintf(stderr, "Error: --pack-inputs is not supported with --follow (a followed file grows; a packed one is whole)\n"); return 1; }
    if (follow && render_gpu) { fprintf(stderr, "Error: --render-on-gpu is not supported with --follow (a followed file's batches continue a line count only the printer knows)\n"); return 1; }
    if (follow && gz_gpu) { fprintf(stderr, "Error: --gz-on-gpu is not supported with --follow (a followed file grows; a gz pack is whole)\n"); return 1; }
    if (follow && stats) fprintf(stderr, "[INFO] Processing existing file content...\n");
    if (follow) for (size_t i = 1; i < pos.size(); ++i) if (pos[i] == "-") { fprintf(stderr, "Error: --follow mode not supported with stdin\n"); return 1; }
    // device list: one worker (scanner) per entry; an entry may repeat (two scanners on one GPU overlap one batch's
    // transfers with the other's kernels)
    std::vector<int> devs;
    if (devices.empty()) devs.push_back(device);
    else if (devices == "all") {
        const int n = matchy_amd_device_count();
        if (n < 1) { fprintf(stderr, "Error: no HIP device available\n"); return 1; }
        for (int d = 0; d < n; ++d) devs.push_back(d);
    } else {
        std::stringstream ss(devices);
        std::string part;
        while (std::getline(ss, part, ',')) {
            part = trim(part);
            if (part.empty() || part.find_first_not_of("0123456789") != std::string::npos) { fprintf(stderr, "Error: bad --devices entry '%s'\n", part.c_str()); return 1; }
            devs.push_back(atoi(part.c_str()));
        }
        if (devs.empty()) { fprintf(stderr, "Error: --devices needs at least one device\n"); return 1; }
    }
    {
        // Workers. A device that is listed once gets several scanners (-j N: N in all, spread over the devices): one scanner's hit
        // post-processing runs under another's transfer (one scanner per GPU: 24 GB/s in the scan phase, two: 44). A device list
        // with repeats is taken as written.
        std::vector<int> uniq = devs;
        std::sort(uniq.begin(), uniq.end());
        const bool repeats = std::adjacent_find(uniq.begin(), uniq.end()) != uniq.end();
        if (!repeats) {
            // auto: two scanners per device keep the bus busy when only counters come back (one copies while the other post-processes);
            // rendering NDJSON is per-hit host work, which four workers share better
            const size_t want = jobs > 0 ? std::max<size_t>((size_t)jobs, devs.size()) : devs.size() * (format == "json" ? 4 : 2);
            const std::vector<int> base = devs;
            for (size_t k = base.size(); k < want; ++k) devs.push_back(base[k % base.size()]);
        }
    }
    const auto t0 = std::chrono::steady_clock::now();
    // database: .mxy file, or a .csv / .json source that is built in memory first (match_cmd.rs:20-31, 222-239)
    matchy_t* db = nullptr;
    const std::string dbpath = pos[0];
    if (ends_with_ci(dbpath, ".csv") || ends_with_ci(dbpath, ".json")) {
        DatabaseBuilder b;
        std::string err;
        std::vector<uint8_t> blob;
        if (!add_inputs(b, {dbpath}, ends_with_ci(dbpath, ".csv") ? "csv" : "json", false, err) || !b.build(blob)) {
            fprintf(stderr, "Error: %s\n", err.empty() ? b.error().c_str() : err.c_str());
            return 1;
        }
        db = matchy_open_buffer(blob.data(), blob.size());
    } else {
        db = matchy_open(dbpath.c_str());
    }
    if (!db) { fprintf(stderr, "Error: Failed to open database %s: %s\n", dbpath.c_str(), matchy_amd_last_error()); return 1; }
    const bool trace = getenv("MATCHY_AMD_TRACE") != nullptr;
    auto since0 = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    if (trace) fprintf(stderr, "[matchy] database open after %.1f ms\n", since0());
    uint32_t mask = 0;
    if (!extractors.empty()) {
        uint32_t auto_mask = 0;
        if (matchy_has_ip_data(db)) auto_mask |= MATCHY_EXTRACT_IPV4 | MATCHY_EXTRACT_IPV6;
        if (matchy_has_literal_data(db) || matchy_has_glob_data(db))
            auto_mask |= MATCHY_EXTRACT_DOMAINS | MATCHY_EXTRACT_EMAILS | MATCHY_EXTRACT_HASHES | MATCHY_EXTRACT_BITCOIN | MATCHY_EXTRACT_ETHEREUM | MATCHY_EXTRACT_MONERO;
        std::string err;
        if (!parse_extractors(extractors, auto_mask, mask, err)) { fprintf(stderr, "Error: %s\n", err.c_str()); matchy_close(db); return 1; }
    }
    // The pipeline: one worker and scanner per device entry inside the library (the first scanner is created here and now, so a device
    // that cannot be used fails the command; the others when the first batch reaches their workers — a small input never pays for
    // scanners it does not use)
    std::vector<int32_t> dev32(devs.begin(), devs.end());
    matchy_multi_scanner_t* ms = matchy_multi_scanner_create(db, mask, dev32.data(), dev32.size());
    if (!ms) {
        fprintf(stderr, "Error: Failed to create the GPU scanner on device %d: %s\n", devs[0], matchy_amd_last_error());
        matchy_close(db);
        return 1;
    }
    const size_t n_scanners = devs.size();
    if (trace) fprintf(stderr, "[matchy] first of %zu scanner(s) created after %.1f ms\n", n_scanners, since0());
    MatchPipeline pl;
    pl.ms = ms;
    pl.json = format == "json";
    // --gz-on-gpu without records to render: no text comes back from a gz pack, so "Lines with matches" is counted on the GPU for every
    // batch (line context; with --format summary it changes nothing that is printed)
    pl.line_ctx = line_numbers || input_line || (gz_gpu && format != "json");
    pl.input_line = input_line;
    pl.gather = gather_lines;
    pl.gz_members = gz_members;
    pl.render_gpu = render_gpu;   // takes effect with --format json only (MatchPipeline::arm)
    if (pl.line_ctx) matchy_multi_scanner_set_line_context(ms, true);
    if (pl.gather) matchy_multi_scanner_set_hit_lines(ms, true);
    if (tally) matchy_multi_scanner_set_tally(ms, true);
    pl.whole_lines = whole_lines;
    if (whole_lines) matchy_multi_scanner_set_whole_lines(ms, true);
    matchy_multi_scanner_set_batch_hook(ms, &MatchPipeline::batch_hook, &pl);
    std::vector<std::string> paths;
    bool stdin_seen = false;
    for (size_t i = 1; i < pos.size(); ++i) {
        if (pos[i] == "-") {
            if (stdin_seen) { if (stats) fprintf(stderr, "[WARN] Skipping duplicate stdin argument\n"); continue; }
            stdin_seen = true;
        }
        paths.push_back(pos[i]);
        pl.sources.push_back(pos[i] == "-" ? "stdin" : pos[i]);
    }
    Totals t;
    std::vector<char> input_failed(paths.size(), 0);
    std::vector<char> read_failed(paths.size(), 0);   // written by this thread only (input_failed belongs to the printer until it is joined)
    pl.line_base.assign(paths.size(), 0);
    std::thread printer([&] { pl.printer(t, input_failed); });
    pl.consumed.assign(paths.size(), -1);
    PackStats packed;
    GzPacker gzp(pl, paths, read_failed, batch_bytes);
    gzp.members = gz_members;
    gzp.windows = gz_windows;
    // an input that is not part of a plain pack: into the gz pack in hand, or, behind that pack and its verdict, the way it is read without the flags
    auto single = [&](size_t i) {
        if (gz_gpu && gzp.take(i)) return;
        if (gz_gpu) gzp.barrier();
        if (gz_windows && gzp.take_windows(i)) return;
        if (!read_input(pl, i, paths[i], batch_bytes)) read_failed[i] = 1;
    };
    if (pack) {
        // runs of small files go out as packs, everything else the way it goes without the flag, in the order of the command line
        packed = pack_inputs(
            paths, batch_bytes,
            [&](InputPack&& p) {
                if (gz_gpu) gzp.barrier();
                Batch b;
                b.input = p.inputs[0].input; b.ptr = p.data.get(); b.len = p.len; b.own = std::move(p.data);
                b.pack = std::move(p.inputs); b.appended = p.appended;
                b.reg = prefault_and_pin(b.ptr, b.len);
                pl.submit(std::move(b));
            },
            single,
            [&](size_t i, int err) { fprintf(stderr, "[ERROR] Failed to process %s: %s\n", paths[i].c_str(), strerror(err)); read_failed[i] = 1; });
    } else {
        for (size_t i = 0; i < paths.size(); ++i) single(i);
    }
    if (gz_gpu) gzp.barrier();
    pl.reader_done = true;
    printer.join();
    for (size_t i = 0; i < paths.size(); ++i) if (read_failed[i]) input_failed[i] = 1;
    for (size_t i : pl.rejected_inputs) if (i < input_failed.size()) input_failed[i] = 1;
    // --tally: the workers' tables merged, one JSON line per distinct matched value behind the match records; what the database holds for
    // a value is asked of it now (a host query per row of the report)
    bool tally_failed = false;
    uint64_t tally_distinct = 0;
    if (tally) {
        matchy_tally_t tl;
        if (matchy_multi_scanner_tally_top(ms, tally_limit, &tl) != MATCHY_SUCCESS) {
            fprintf(stderr, "Error: Failed to read the hit tally: %s\n", matchy_amd_last_error());
            tally_failed = true;
        } else {
            tally_distinct = tl.distinct;
            std::string line;
            for (size_t i = 0; i < tl.n_entries; ++i) {
                const matchy_tally_entry_t& e = tl.entries[i];
                const std::string text((const char*)e.text, e.len);
                line = "{\"count\":" + std::to_string((unsigned long long)e.count) + ",\"item_type\":";
                json_escape(matchy_item_type_name(e.item_type), line);
                line += ",\"matched_text\":";
                json_escape(text, line);
                line += ",\"result\":";
                int32_t found = 0;
                char* js = matchy_amd_query_json(db, text.c_str(), &found);
                line += js ? js : "[]";
                if (js) matchy_free_string(js);
                line += "}\n";
                fwrite(line.data(), 1, line.size(), stdout);
            }
            matchy_tally_free(&tl);
        }
    }
    fflush(stdout);
    if (trace) fprintf(stderr, "[matchy] all batches done after %.1f ms\n", since0());
    pl.release_mappings((size_t)-1);
    if (follow) {
        matchy_scanner_t* fsc = matchy_scanner_create(db, mask, devs[0]);
        if (!fsc) fprintf(stderr, "Error: Failed to create the GPU scanner on device %d: %s\n", devs[0], matchy_amd_last_error());
        else { matchy_scanner_set_line_context(fsc, pl.line_ctx); matchy_scanner_set_hit_lines(fsc, pl.gather); matchy_scanner_set_whole_lines(fsc, whole_lines); follow_inputs(pl, fsc, paths, stats, t); matchy_scanner_free(fsc); }
    }
    size_t failed = 0;
    for (char f : input_failed) failed += f != 0;
    const size_t processed = paths.size() - failed;
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (stats) {
        fprintf(stderr, "\n[INFO] === Processing Complete ===\n");
        if (pos.size() > 2) {
            fprintf(stderr, "[INFO] Files processed: %zu\n", processed);
            if (failed) fprintf(stderr, "[INFO] Files failed: %zu\n", failed);
        }
        fprintf(stderr, "[INFO] Lines processed: %s\n", fmt_num(t.lines).c_str());
        fprintf(stderr, "[INFO] Lines with matches: %s (%.1f%%)\n", fmt_num(t.lines_with_matches).c_str(),
                t.lines ? 100.0 * (double)t.lines_with_matches / (double)t.lines : 0.0);
        fprintf(stderr, "[INFO] Total matches: %s\n", fmt_num(t.matches).c_str());
        fprintf(stderr, "[INFO] Candidates tested: %s\n", fmt_num(t.candidates).c_str());
        if (whole_lines) fprintf(stderr, "[INFO] Whole-line queries: %s (%s addresses, %s strings, %s not valid UTF-8)\n", fmt_num(pl.wl_counters[0].load()).c_str(),
                                 fmt_num(pl.wl_counters[1].load()).c_str(), fmt_num(pl.wl_counters[2].load()).c_str(), fmt_num(pl.wl_counters[3].load()).c_str());
        if (tally && !tally_failed) fprintf(stderr, "[INFO] Distinct matched values: %s\n", fmt_num(tally_distinct).c_str());
        fprintf(stderr, "[INFO] Throughput: %.2f MB/s\n", secs > 0 ? (double)t.bytes / 1e6 / secs : 0.0);
        fprintf(stderr, "[INFO] Total time: %.2fs\n", secs);
        fprintf(stderr, "[INFO] Query rate: %.0f queries/s\n", secs > 0 ? (double)t.candidates / secs : 0.0);
        std::string dl;
        for (int d : devs) { if (!dl.empty()) dl += ","; dl += std::to_string(d); }
        fprintf(stderr, "\n[INFO] === Devices ===\n[INFO] HIP devices: %s (%zu scanner%s, batches of %zu MiB)\n", dl.c_str(), n_scanners,
                n_scanners == 1 ? "" : "s", batch_bytes >> 20);
        if (render_gpu) fprintf(stderr, "[INFO] Rendered %zu batches on the GPU (%llu bytes of NDJSON), %zu fell back to the host renderer\n", pl.gpu_batches.load(), pl.gpu_bytes.load(), pl.gpu_fallback.load());
        if (pack) fprintf(stderr, "[INFO] Packed %zu inputs into %zu batches (%llu bytes of input in all)\n", packed.inputs, packed.packs, t.bytes);
        if (gz_gpu) fprintf(stderr, "[INFO] Inflated %zu .gz inputs on the GPU in %zu batches (%llu -> %llu bytes), %zu read on the host\n", gzp.on_gpu, gzp.packs,
                            gzp.packed_bytes, gzp.text_bytes, gzp.on_host);
        if (gz_members) fprintf(stderr, "[INFO] gz members on the GPU: %zu in %zu multi-member files\n", gzp.multi_members, gzp.multi_files);
        if (gz_windows) fprintf(stderr, "[INFO] gz windows on the GPU: %zu windows of %zu files, %zu finished on the host\n", gzp.win_windows, gzp.win_files, gzp.win_host);
    }
    matchy_multi_scanner_free(ms);
    matchy_close(db);
    if (trace) fprintf(stderr, "[matchy] cleaned up after %.1f ms\n", since0());
    if (failed) { fprintf(stderr, "Error: %zu file(s) failed to process\n", failed); return 1; }
    return tally_failed ? 1 : 0;
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
bool extract_batch(matchy_extractor_t* ex, uint8_t* data, size_t len, int fmt, bool show_cand, ExtractStats& st) {
    if (!len) return true;
    // line table: [start, end) of every trimmed, non-empty line
    std::vector<std::pair<size_t, size_t>> lines;
    for (size_t p = 0; p < len;) {
        const uint8_t* nlp = (const uint8_t*)memchr(data + p, '\n', len - p);
        size_t e = nlp ? (size_t)(nlp - data) : len, a = p, b = e;
        while (a < b && is_ws(data[a])) { if (data[a] == 0x0C) data[a] = ' '; ++a; }
        while (b > a && is_ws(data[b - 1])) { if (data[b - 1] == 0x0C) data[b - 1] = ' '; --b; }
        if (b > a) { lines.push_back({a, b}); st.lines++; st.bytes += b - a; }
        p = e + 1;
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
    bool have_types = false, unique = false, stats = false, show_cand = false;
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
        else if (a.size() > 1 && a[0] == '-') { fprintf(stderr, "error: unexpected argument '%s'\n", a.c_str()); return 2; }
        else inputs.push_back(a);
    }
    if (inputs.empty()) return usage();
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
            return extract_batch(ex, data.get(), len, fmt, show_cand, st);
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
