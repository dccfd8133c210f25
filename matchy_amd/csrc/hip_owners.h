// Errors and owners of HIP resources: device memory, pinned host memory, events, streams. Every owner releases what it holds in its
// destructor and cannot be copied or moved, so a class that has one as a member needs no release code of its own. Nothing here knows
// about scans.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>
#include <utility>
#include <vector>

namespace mxy {

struct HipError { std::string what; };
// what the caller handed in cannot be scanned (a segment table that breaks its rules): nothing is wrong with the device or the scanner
struct ParamError { std::string what; };
#define MXY_HIP(expr)                                                                                   \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess) throw ::mxy::HipError{std::string(#expr) + ": " + hipGetErrorString(_e)}; \
    } while (0)

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    void alloc(size_t count) {
        free();
        if (count) MXY_HIP(hipMalloc((void**)&p, count * sizeof(T)));
        n = count;
    }
    void upload(const std::vector<T>& v) { alloc(v.size()); if (!v.empty()) MXY_HIP(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice)); }
    void free() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
    // allocate into a fresh buffer, fill it, then swap: the old content stays valid until the new one is complete
    void swap(DevBuf& o) { std::swap(p, o.p); std::swap(n, o.n); }
    ~DevBuf() { free(); }
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
};

// Pinned host memory (hipHostMalloc). Between the release of the old block and the success of the new allocation the pointer is null
// and the size is zero: an allocation that throws leaves an empty buffer behind, never a dangling one.
template <class T>
struct PinnedBuf {
    T* p = nullptr;
    size_t n = 0;
    void alloc(size_t count) {
        free();
        if (count) MXY_HIP(hipHostMalloc((void**)&p, count * sizeof(T), hipHostMallocDefault));
        n = count;
    }
    // room for `count` elements; a block that is too small is replaced by one of count + slack (its content is not kept)
    void ensure(size_t count, size_t slack = 0) { if (n < count) alloc(count + slack); }
    void free() { if (p) (void)hipHostFree(p); p = nullptr; n = 0; }
    ~PinnedBuf() { free(); }
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
};

// One event / one stream. Empty until create(), which the owner of the member calls where the handle is first needed; a second
// create() keeps the handle there is.
class Event {
public:
    Event() = default;
    ~Event() { if (e_) (void)hipEventDestroy(e_); }
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    void create(unsigned flags = hipEventDefault) { if (!e_) MXY_HIP(hipEventCreateWithFlags(&e_, flags)); }
    operator hipEvent_t() const { return e_; }
private:
    hipEvent_t e_ = nullptr;
};

class Stream {
public:
    Stream() = default;
    ~Stream() { if (s_) (void)hipStreamDestroy(s_); }
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    void create(unsigned flags = hipStreamNonBlocking) { if (!s_) MXY_HIP(hipStreamCreateWithFlags(&s_, flags)); }
    operator hipStream_t() const { return s_; }
private:
    hipStream_t s_ = nullptr;
};

}  // namespace mxy
