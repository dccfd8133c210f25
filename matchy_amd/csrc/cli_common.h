// What the files of the `matchy` command line share (cli_main.cpp: main and the small commands; cli_match.cpp: `matchy match`).
#pragma once
#include <cerrno>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/matchy_amd.h"
#include "data_codec.h"
#include "db_builder.h"

int usage();
int cmd_match(int argc, char** argv);

namespace mxy {
inline bool ends_with_ci(const std::string& s, const char* suf) {
    size_t n = strlen(suf);
    if (s.size() < n) return false;
    for (size_t i = 0; i < n; ++i) if (tolower((unsigned char)s[s.size() - n + i]) != suf[i]) return false;
    return true;
}

inline std::string fmt_num(unsigned long long v) {  // 1234567 -> "1,234,567" (bin/cli_utils.rs:143-153)
    std::string s = std::to_string(v), out;
    for (size_t i = 0; i < s.size(); ++i) {
        if (i && (s.size() - i) % 3 == 0) out.push_back(',');
        out.push_back(s[i]);
    }
    return out;
}

inline std::string trim(const std::string& s) {
    size_t a = 0, b = s.size();
    while (a < b && isspace((unsigned char)s[a])) ++a;
    while (b > a && isspace((unsigned char)s[b - 1])) --b;
    return s.substr(a, b - a);
}

// One CSV record (RFC 4180 quoting as the `csv` crate reads it by default: quotes, doubled quotes, embedded newlines).
inline bool read_csv_record(std::istream& in, std::vector<std::string>& out) {
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
inline DataValue csv_value(const std::string& v) {
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

inline bool add_inputs(DatabaseBuilder& b, const std::vector<std::string>& inputs, const std::string& format, bool verbose, std::string& err) {
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

// --extractors=ip,domain / -crypto,-hash ... (bin/matchy.rs:124-131): returns the MATCHY_EXTRACT_* mask, 0 = auto
inline bool parse_extractors(const std::string& spec, uint32_t auto_mask, uint32_t& mask, std::string& err) {
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

}  // namespace mxy
