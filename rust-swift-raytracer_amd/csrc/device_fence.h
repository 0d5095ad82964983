// device_fence.h -- owners of events and streams, and the fence that orders
// work enqueued on different streams.
//
// The only place in csrc/ that creates or destroys either kind.  An owner
// destroys its handle when it goes out of scope (errors ignored, as in
// device_buffer.h) and makes no HIP call on a null handle, so a struct that is
// created and freed without a GPU never touches the runtime.
#pragma once

#include <hip/hip_runtime.h>

#include <utility>

namespace rtamd {

// A HIP handle destroyed by Destroy.  Move-only; empty is nullptr.
template <typename H, hipError_t (*Destroy)(H)>
class DevHandle {
public:
    DevHandle() = default;
    DevHandle(const DevHandle &) = delete;
    DevHandle &operator=(const DevHandle &) = delete;
    DevHandle(DevHandle &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    DevHandle &operator=(DevHandle &&o) noexcept {  // (o takes the old handle with it)
        std::swap(h_, o.h_);
        return *this;
    }
    ~DevHandle() { reset(); }

    H get() const { return h_; }
    explicit operator bool() const { return h_ != nullptr; }

    void reset() {
        if (h_) (void)Destroy(h_);
        h_ = nullptr;
    }

protected:
    H h_ = nullptr;
};

// An event of the device that is current at create (a no-op once it exists).
// timing: for hipEventElapsedTime; without, the cheaper kind that only orders.
class DevEvent : public DevHandle<hipEvent_t, hipEventDestroy> {
public:
    hipError_t create(bool timing) {
        if (h_) return hipSuccess;
        return timing ? hipEventCreate(&h_) : hipEventCreateWithFlags(&h_, hipEventDisableTiming);
    }
};

// A non-blocking stream of the device that is current at create (a no-op once it exists).
class DevStream : public DevHandle<hipStream_t, hipStreamDestroy> {
public:
    hipError_t create() { return h_ ? hipSuccess : hipStreamCreateWithFlags(&h_, hipStreamNonBlocking); }
    // ... at the lowest priority the device offers: work that fills what other streams leave idle
    hipError_t create_lowest_priority() {
        if (h_) return hipSuccess;
        int least = 0, greatest = 0;
        const hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);
        return e != hipSuccess ? e : hipStreamCreateWithPriority(&h_, hipStreamNonBlocking, least);
    }
};

// The end of the last work enqueued on something shared, and the stream it
// went to: whoever enqueues more on another stream waits for it first, and
// records it again behind the work.  The destructor does not wait: an owner
// whose buffers the recorded work may still use calls sync() before they go.
class Fence {
public:
    // s waits for the recorded work (nothing recorded, or recorded on s: no call)
    hipError_t wait(hipStream_t s) const {
        if (!recorded_ || stream_ == s) return hipSuccess;
        return hipStreamWaitEvent(s, ev_.get(), 0);
    }
    // the work enqueued on s so far (the event is created here, on the current device)
    hipError_t record(hipStream_t s) {
        hipError_t e = ev_.create(false);
        if (e == hipSuccess) e = hipEventRecord(ev_.get(), s);
        if (e != hipSuccess) return e;
        stream_ = s;
        recorded_ = true;
        return hipSuccess;
    }
    // the host waits for the recorded work (nothing recorded: no call)
    hipError_t sync() const { return recorded_ ? hipEventSynchronize(ev_.get()) : hipSuccess; }
    bool recorded() const { return recorded_; }

private:
    DevEvent ev_;
    hipStream_t stream_ = nullptr;
    bool recorded_ = false;
};

}  // namespace rtamd
