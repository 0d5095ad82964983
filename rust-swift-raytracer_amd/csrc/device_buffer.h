// device_buffer.h -- owners of device and pinned host memory.
//
// The only place in csrc/ that allocates or frees either kind.  A buffer
// frees its memory when it goes out of scope (errors ignored: nothing can be
// done about them there), so a struct of buffers needs no list of what to free.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <vector>

namespace rtamd {

// cap elements of T in device memory (Pinned: in page-locked host memory).
// Move-only.  A null get() is read as a flag in several places (runtime.h),
// so an empty buffer is always {nullptr, 0}.
template <typename T, bool Pinned = false>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : ptr_(o.ptr_), cap_(o.cap_), pinned_(o.pinned_) {
        o.ptr_ = nullptr; o.cap_ = 0; o.pinned_ = false;
    }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            reset();
            ptr_ = o.ptr_; cap_ = o.cap_; pinned_ = o.pinned_;
            o.ptr_ = nullptr; o.cap_ = 0; o.pinned_ = false;
        }
        return *this;
    }
    ~DevBuf() { reset(); }

    T *get() const { return ptr_; }
    size_t cap() const { return cap_; }
    explicit operator bool() const { return ptr_ != nullptr; }

    void reset() {
        if (ptr_) (void)(Pinned ? hipHostFree(ptr_) : hipFree(ptr_));
        ptr_ = nullptr;
        cap_ = 0;
        pinned_ = false;
    }

    // Held: a graph's nodes name this memory (a captured frame bound it), so its
    // owner moves the buffer aside instead of rewriting, growing or freeing it
    // (runtime.h DeviceState::retire).  The mark goes with the memory.
    void hold() { pinned_ = ptr_ != nullptr; }
    bool held() const { return pinned_; }

    // Room for n elements: a no-op when n <= cap(), else the old memory is
    // freed and new memory allocated (contents discarded); empty on failure.
    hipError_t grow(size_t n) {
        if (n <= cap_) return hipSuccess;
        reset();
        const hipError_t e = Pinned ? hipHostMalloc((void **)&ptr_, n * sizeof(T))
                                    : hipMalloc((void **)&ptr_, n * sizeof(T));
        if (e == hipSuccess) cap_ = n;
        else ptr_ = nullptr;
        return e;
    }

    // src to the start of the buffer with a synchronous copy (src may be
    // pageable and change right after the call), grown to hold src or
    // min_elems elements of U, whichever is more.  U need not be T: vectors
    // of words fill buffers of float4 or uint4 records.
    template <typename U>
    hipError_t upload(const std::vector<U> &src, size_t min_elems = 0) {
        const size_t bytes = std::max(src.size(), min_elems) * sizeof(U);
        const hipError_t e = grow((bytes + sizeof(T) - 1) / sizeof(T));
        if (e != hipSuccess || src.empty()) return e;
        return hipMemcpy(ptr_, src.data(), src.size() * sizeof(U),
                         Pinned ? hipMemcpyHostToHost : hipMemcpyHostToDevice);
    }

private:
    T *ptr_ = nullptr;
    size_t cap_ = 0;
    bool pinned_ = false;
};

template <typename T>
using PinnedBuf = DevBuf<T, true>;

}  // namespace rtamd
