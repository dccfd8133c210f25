// IP address text <-> binary helpers with Rust std semantics (the reference parses keys with
// `str::parse::<IpAddr>()`, crates/matchy-format/src/mmdb_builder.rs:338-365, and prints with Display). Parsing and the
// formatting into a caller's buffer (format_*_to) are host/device code: the NDJSON renderer on the GPU (render_core.h) uses
// the same definitions as the host. The std::string forms wrap them.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MXY_ADDR_HD __host__ __device__ inline
#else
#define MXY_ADDR_HD inline
#endif

namespace mxy {

struct IpAddr {
    bool v6 = false;
    uint8_t b[16] = {0};  // v4: b[0..4]
};

// room for any text format_cidr_to writes: 39 bytes of IPv6, '/', and a 32-bit prefix in decimal
constexpr uint32_t IP_CIDR_TEXT_MAX = 56;

namespace detail {
// Every loop of the parser is bounded by its digit limits and the eight groups, not by n: a text of any length costs the same.
struct AddrParser {
    const char* s;
    size_t n, pos = 0;
    // read_number(radix, max_digits, allow_zero_prefix) — atomic
    MXY_ADDR_HD bool number(int radix, int max_digits, bool allow_zero_prefix, uint32_t maxval, uint32_t& out) {
        size_t p = pos;
        uint32_t v = 0;
        int digits = 0;
        bool leading_zero = p < n && s[p] == '0';
        while (p < n) {
            char c = s[p];
            int d;
            if (c >= '0' && c <= '9') d = c - '0';
            else if (radix == 16 && c >= 'a' && c <= 'f') d = c - 'a' + 10;
            else if (radix == 16 && c >= 'A' && c <= 'F') d = c - 'A' + 10;
            else break;
            v = v * radix + d;
            ++digits;
            ++p;
            if (digits > max_digits) return false;
        }
        if (digits == 0) return false;
        if (!allow_zero_prefix && leading_zero && digits > 1) return false;
        if (v > maxval) return false;
        out = v;
        pos = p;
        return true;
    }
    MXY_ADDR_HD bool ipv4(uint8_t o[4]) {
        size_t save = pos;
        for (int i = 0; i < 4; ++i) {
            if (i > 0) {
                if (pos < n && s[pos] == '.') ++pos;
                else { pos = save; return false; }
            }
            uint32_t v;
            if (!number(10, 3, false, 255, v)) { pos = save; return false; }
            o[i] = (uint8_t)v;
        }
        return true;
    }
    // read_groups: returns (count, ends_with_ipv4)
    MXY_ADDR_HD size_t groups(uint16_t* g, size_t limit, bool& v4) {
        v4 = false;
        for (size_t i = 0; i < limit; ++i) {
            if (i + 1 < limit) {  // try a trailing embedded IPv4 (needs two groups)
                size_t save = pos;
                bool ok = true;
                if (i > 0) { if (pos < n && s[pos] == ':') ++pos; else ok = false; }
                uint8_t o[4];
                if (ok && ipv4(o)) {
                    g[i] = (uint16_t)((o[0] << 8) | o[1]);
                    g[i + 1] = (uint16_t)((o[2] << 8) | o[3]);
                    v4 = true;
                    return i + 2;
                }
                pos = save;
            }
            size_t save = pos;
            if (i > 0) { if (pos < n && s[pos] == ':') ++pos; else { pos = save; return i; } }
            uint32_t v;
            if (!number(16, 4, true, 0xFFFF, v)) { pos = save; return i; }
            g[i] = (uint16_t)v;
        }
        return limit;
    }
    MXY_ADDR_HD bool ipv6(uint16_t seg[8]) {
        uint16_t head[8] = {0};
        bool head_v4;
        size_t hs = groups(head, 8, head_v4);
        if (hs == 8) { for (int i = 0; i < 8; ++i) seg[i] = head[i]; return true; }
        if (head_v4) return false;
        if (!(pos < n && s[pos] == ':')) return false;
        ++pos;
        if (!(pos < n && s[pos] == ':')) return false;
        ++pos;
        uint16_t tail[7] = {0};
        bool tv4;
        size_t limit = 8 - (hs + 1);
        size_t ts = groups(tail, limit, tv4);
        for (size_t i = 0; i < ts; ++i) head[8 - ts + i] = tail[i];
        for (int i = 0; i < 8; ++i) seg[i] = head[i];
        return true;
    }
};

// v in decimal / lower-case hex without leading zeros; returns the number of characters (at most 10 / 4)
MXY_ADDR_HD uint32_t put_u32_dec(uint32_t v, char* o) {
    uint32_t n = 1;
    for (uint32_t t = v; t >= 10; t /= 10) ++n;
    for (uint32_t k = n; k-- > 0; v /= 10) o[k] = (char)('0' + v % 10);
    return n;
}
MXY_ADDR_HD uint32_t put_u16_hex(uint32_t v, char* o) {
    uint32_t n = 1;
    for (uint32_t t = v; t >= 16; t /= 16) ++n;
    for (uint32_t k = n; k-- > 0; v /= 16) o[k] = (char)((v & 15) < 10 ? '0' + (v & 15) : 'a' + ((v & 15) - 10));
    return n;
}
}  // namespace detail

MXY_ADDR_HD bool parse_ipv4(const char* s, size_t n, uint8_t out[4]) {
    detail::AddrParser p{s, n};
    return p.ipv4(out) && p.pos == n;
}
MXY_ADDR_HD bool parse_ipv6(const char* s, size_t n, uint8_t out[16]) {
    detail::AddrParser p{s, n};
    uint16_t seg[8];
    if (!p.ipv6(seg) || p.pos != n) return false;
    for (int i = 0; i < 8; ++i) { out[2 * i] = (uint8_t)(seg[i] >> 8); out[2 * i + 1] = (uint8_t)seg[i]; }
    return true;
}
MXY_ADDR_HD bool parse_ip(const char* s, size_t n, IpAddr& a) {
    a = IpAddr();
    if (parse_ipv4(s, n, a.b)) { a.v6 = false; return true; }
    if (parse_ipv6(s, n, a.b)) { a.v6 = true; return true; }
    return false;
}

// The *_to forms write into `o` (no terminator) and return the length: at most 15, 39 and IP_CIDR_TEXT_MAX characters.
MXY_ADDR_HD uint32_t format_ipv4_to(const uint8_t a[4], char* o) {
    uint32_t n = 0;
    for (int i = 0; i < 4; ++i) {
        if (i) o[n++] = '.';
        n += detail::put_u32_dec(a[i], o + n);
    }
    return n;
}
// <Ipv6Addr as Display>: "::ffff:a.b.c.d" for IPv4-mapped, otherwise RFC 5952 (longest zero run >= 2 compressed, first wins)
MXY_ADDR_HD uint32_t format_ipv6_to(const uint8_t a[16], char* o) {
    uint16_t seg[8];
    for (int i = 0; i < 8; ++i) seg[i] = (uint16_t)((a[2 * i] << 8) | a[2 * i + 1]);
    uint32_t n = 0;
    if (!seg[0] && !seg[1] && !seg[2] && !seg[3] && !seg[4] && seg[5] == 0xffff) {
        const char* lead = "::ffff:";
        for (int i = 0; i < 7; ++i) o[n++] = lead[i];
        return n + format_ipv4_to(a + 12, o + n);
    }
    int bs = 0, bl = 0, cs = 0, cl = 0;
    for (int i = 0; i < 8; ++i) {
        if (seg[i] == 0) { if (cl == 0) cs = i; ++cl; if (cl > bl) { bl = cl; bs = cs; } }
        else cl = 0;
    }
    if (bl <= 1) { bs = 8; bl = 0; }   // nothing to compress: one run of eight groups
    for (int i = 0; i < bs; ++i) { if (i) o[n++] = ':'; n += detail::put_u16_hex(seg[i], o + n); }
    if (bs == 8) return n;
    o[n++] = ':'; o[n++] = ':';
    for (int i = bs + bl; i < 8; ++i) { if (i > bs + bl) o[n++] = ':'; n += detail::put_u16_hex(seg[i], o + n); }
    return n;
}
MXY_ADDR_HD uint32_t format_ip_to(const IpAddr& a, char* o) { return a.v6 ? format_ipv6_to(a.b, o) : format_ipv4_to(a.b, o); }

// format_cidr_into (crates/matchy/src/bin/cli_utils.rs:107-141)
MXY_ADDR_HD uint32_t format_cidr_to(const IpAddr& a, unsigned prefix, char* o) {
    IpAddr net = a;
    int nb = a.v6 ? 16 : 4;
    for (int i = 0; i < nb; ++i) {
        int left = (int)prefix - i * 8;
        uint8_t mask = left >= 8 ? 0xFF : left <= 0 ? 0 : (uint8_t)(0xFF << (8 - left));
        net.b[i] &= mask;
    }
    uint32_t n = format_ip_to(net, o);
    o[n++] = '/';
    return n + detail::put_u32_dec(prefix, o + n);
}

inline std::string format_ipv4(const uint8_t a[4]) { char b[IP_CIDR_TEXT_MAX]; return std::string(b, format_ipv4_to(a, b)); }
inline std::string format_ipv6(const uint8_t a[16]) { char b[IP_CIDR_TEXT_MAX]; return std::string(b, format_ipv6_to(a, b)); }
inline std::string format_ip(const IpAddr& a) { return a.v6 ? format_ipv6(a.b) : format_ipv4(a.b); }
inline std::string format_cidr(const IpAddr& a, unsigned prefix) { char b[IP_CIDR_TEXT_MAX]; return std::string(b, format_cidr_to(a, prefix, b)); }

}  // namespace mxy
