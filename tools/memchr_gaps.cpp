// The host-side "lines with matches" loop of `matchy match` (MatchPipeline::render in cli_match.cpp) as a function, for
// tools/line_context_timing.py: hit starts sorted by offset; a new line starts when a '\n' lies between two hit starts.
#include <cstddef>
#include <cstdint>
#include <cstring>

extern "C" unsigned long long memchr_gaps(const uint8_t* data, const uint32_t* starts, size_t n) {
    unsigned long long lines_with_matches = 0;
    size_t prev = (size_t)-1;
    for (size_t i = 0; i < n; ++i) {
        const size_t s = starts[i];
        if (prev == (size_t)-1 || memchr(data + prev, '\n', s - prev)) ++lines_with_matches;
        prev = s;
    }
    return lines_with_matches;
}
