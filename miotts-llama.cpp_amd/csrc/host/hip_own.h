// Move-only owners of the HIP handles the LLM runner holds, and the one stream capture
// (capture_graph). Nothing else: errors stay with MIO_HIP_CHECK (common.h).
#pragma once

#include <utility>

#include "common.h"

#pragma GCC visibility push(hidden)
namespace mio {

// A handle released by Free when its owner goes away. Reads convert to the handle itself;
// put() is the out-parameter of the call that creates it (what was held is released first).
template <class T, auto Free>
class HipOwn {
    T h_{};

public:
    HipOwn() = default;
    HipOwn(HipOwn &&o) noexcept : h_(std::exchange(o.h_, T{})) {}
    HipOwn &operator=(HipOwn &&o) noexcept {
        if (this != &o) reset(), h_ = std::exchange(o.h_, T{});
        return *this;
    }
    HipOwn(const HipOwn &) = delete;
    HipOwn &operator=(const HipOwn &) = delete;
    ~HipOwn() { reset(); }
    void reset() {
        if (h_) (void)Free(h_);
        h_ = T{};
    }
    T get() const { return h_; }
    operator T() const { return h_; }
    T *put() {
        reset();
        return &h_;
    }
};

using Event = HipOwn<hipEvent_t, hipEventDestroy>;
using GraphExec = HipOwn<hipGraphExec_t, hipGraphExecDestroy>;
template <class T>
using Pinned = HipOwn<T *, hipHostFree>;  // hipHostMalloc memory
template <class T>
using Scratch = HipOwn<T *, hipFree>;  // a hipMalloc block that lives for one call

// Captures what issue() enqueues on s and instantiates it into *out. A capture that began is
// always ended and its hipGraph_t always destroyed; returns issue's error, or else the HIP
// error (*out stays null on either).
template <class F>
int capture_graph(hipStream_t s, F &&issue, hipGraphExec_t *out) {
    MIO_HIP_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    const int rc = issue();
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamEndCapture(s, &g);
    if (rc == MIO_OK && e == hipSuccess) e = hipGraphInstantiate(out, g, nullptr, nullptr, 0);
    if (g) hipGraphDestroy(g);
    if (rc) return rc;
    MIO_HIP_CHECK(e);
    return MIO_OK;
}

}  // namespace mio
#pragma GCC visibility pop
