// Bytes -> UTF-8 text the way Rust's String::from_utf8_lossy does it: well-formed sequences are copied, every maximal ill-formed
// subsequence (Unicode 3.9, "substitution of maximal subparts") becomes one U+FFFD. Header-only so that a CPU test can reach it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

namespace mxy {

inline void utf8_lossy_append(const uint8_t* s, size_t n, std::string& out) {
    size_t i = 0;
    while (i < n) {
        const uint8_t c = s[i];
        if (c < 0x80) {   // the common case: a run of ASCII
            size_t j = i + 1;
            while (j < n && s[j] < 0x80) ++j;
            out.append(reinterpret_cast<const char*>(s) + i, j - i);
            i = j;
            continue;
        }
        size_t need = 0;   // continuation bytes
        uint8_t lo = 0x80, hi = 0xBF;   // range of the first continuation byte
        if (c >= 0xC2 && c <= 0xDF) need = 1;
        else if (c >= 0xE0 && c <= 0xEF) { need = 2; if (c == 0xE0) lo = 0xA0; if (c == 0xED) hi = 0x9F; }
        else if (c >= 0xF0 && c <= 0xF4) { need = 3; if (c == 0xF0) lo = 0x90; if (c == 0xF4) hi = 0x8F; }
        size_t k = 1;   // bytes of the sequence that are well-formed so far
        bool ok = need != 0;
        for (; ok && k <= need; ++k) {
            if (i + k >= n) { ok = false; break; }
            const uint8_t b = s[i + k];
            if (k == 1 ? (b < lo || b > hi) : ((b & 0xC0) != 0x80)) { ok = false; break; }
        }
        if (ok) out.append(reinterpret_cast<const char*>(s) + i, need + 1);
        else out += "\xEF\xBF\xBD";
        i += ok ? need + 1 : k;   // an ill-formed subsequence ends in front of the byte that broke it
    }
}

}  // namespace mxy
