// `matchy match --pack-inputs`: consecutive small input files share a batch. The packer walks the inputs in command-line order, reads
// runs of eligible files end to end into one owned buffer — a '\n' behind a file that lacks a final one, so that every file is a
// newline-terminated segment of the batch (matchy_scanner_set_segments) — and hands everything else back to be read the way it is read
// without the flag, in the same order. Host only (no HIP include) and header-only, like batch_reader.h: the unit test builds this file
// with nothing else.
#pragma once

#include <cerrno>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include "batch_reader.h"

namespace mxy {

// One file of a pack: its index among the inputs, where its segment starts in the pack, and whether a '\n' was appended behind it.
struct PackedInput { size_t input; uint32_t start; bool appended; };
// data[0, len) with 16 spare bytes behind, the files in input order; `appended` counts the added newlines.
struct InputPack { Bytes data; size_t len = 0; std::vector<PackedInput> inputs; size_t appended = 0; };
struct PackStats { size_t inputs = 0, packs = 0; };   // files that went into packs, and the packs

inline bool pack_ends_with_gz(const std::string& s) {
    return s.size() >= 3 && s[s.size() - 3] == '.' && (s[s.size() - 2] | 0x20) == 'g' && (s[s.size() - 1] | 0x20) == 'z';
}

// A regular file that is not "-" and not .gz with 0 < size <= batch_bytes / 4.
inline bool pack_eligible(const std::string& path, size_t batch_bytes, size_t& size) {
    if (path == "-" || pack_ends_with_gz(path)) return false;
    struct stat sb;
    if (stat(path.c_str(), &sb) != 0 || !S_ISREG(sb.st_mode) || sb.st_size <= 0) return false;
    size = (size_t)sb.st_size;
    return size <= batch_bytes / 4;
}

// Reads up to `size` bytes of `path` to dst; the bytes read, or -1 with errno set.
inline long long pack_read_file(const std::string& path, uint8_t* dst, size_t size) {
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) return -1;
    size_t have = 0;
    while (have < size) {
        const ssize_t r = read(fd, dst + have, size - have);
        if (r < 0) { if (errno == EINTR) continue; const int e = errno; close(fd); errno = e; return -1; }
        if (r == 0) break;   // the file shrank behind the stat
        have += (size_t)r;
    }
    close(fd);
    return (long long)have;
}

// on_pack(InputPack&&): a pack of two or more files. on_single(input): read this input the way it is read without packing (not
// eligible, or a pack of one file). on_error(input, errno): an eligible file that could not be opened or read — it does not stop the
// pack. Calls come in input order; a pack goes out when the next file would pass batch_bytes, in front of an input that is not
// eligible, and at the end.
template <class OnPack, class OnSingle, class OnError>
PackStats pack_inputs(const std::vector<std::string>& paths, size_t batch_bytes, OnPack on_pack, OnSingle on_single, OnError on_error) {
    const size_t SPARE = 16;
    PackStats st;
    InputPack cur;
    auto flush = [&] {
        if (cur.inputs.size() == 1) on_single(cur.inputs[0].input);
        else if (cur.inputs.size() > 1) { st.inputs += cur.inputs.size(); ++st.packs; on_pack(std::move(cur)); }
        cur = InputPack();
    };
    for (size_t i = 0; i < paths.size(); ++i) {
        size_t size = 0;
        if (!pack_eligible(paths[i], batch_bytes, size)) { flush(); on_single(i); continue; }
        if (!cur.inputs.empty() && cur.len + size > batch_bytes) flush();
        if (!cur.data) {
            cur.data.reset((uint8_t*)malloc(batch_bytes + SPARE));
            if (!cur.data) { on_error(i, ENOMEM); continue; }
        }
        const long long got = pack_read_file(paths[i], cur.data.get() + cur.len, size);
        if (got < 0) { on_error(i, errno); continue; }
        if (got == 0) continue;   // emptied behind the stat: contributes nothing
        const bool add = cur.data[cur.len + (size_t)got - 1] != '\n';
        if (!cur.inputs.empty() && cur.len + (size_t)got + (add ? 1 : 0) > batch_bytes) {
            // the file fits and the newline it needs does not: it opens the next pack
            Bytes next((uint8_t*)malloc(batch_bytes + SPARE));
            if (!next) { on_error(i, ENOMEM); continue; }
            memcpy(next.get(), cur.data.get() + cur.len, (size_t)got);
            flush();
            cur.data = std::move(next);
        }
        PackedInput pi{i, (uint32_t)cur.len, add};
        cur.len += (size_t)got;
        if (add) { cur.data[cur.len++] = '\n'; ++cur.appended; }
        cur.inputs.push_back(pi);
    }
    flush();
    return st;
}

}  // namespace mxy
