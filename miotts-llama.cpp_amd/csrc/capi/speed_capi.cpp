// C-ABI: the speaking rate (include/mio_hip.h, "speaking rate"): argument checks, the sizes, the
// device's workspace (window + offsets) and the two launches of pcm_speed.hip.
#include "common.h"
#include "pcm_speed.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace {

constexpr long long kMaxSamples = 1LL << 30;  // frame starts and offsets stay far inside 32 bits

long long out_len(long long n, float speed) { return (long long)std::ceil((double)n / (double)speed); }
long long frames_of(long long n_out) { return (n_out + mio::SP_HS - 1) / mio::SP_HS + 1; }

// the window, then SP_MAX_B rows of `frames` offsets. Growing frees the old block (hipFree waits
// for the device, so no launch still reads it); a run inside the reserved size allocates nothing.
int ensure_ws(mio_hip_device *d, long long frames) {
    if (d->speed_ws && d->speed_frames >= frames) return MIO_OK;
    frames = std::max(frames, 2 * d->speed_frames);
    if (d->speed_ws) MIO_HIP_CHECK(hipFree(d->speed_ws));
    d->speed_ws = nullptr, d->speed_frames = 0;
    const size_t bytes = sizeof(float) * mio::SP_N + sizeof(int) * (size_t)mio::SP_MAX_B * (size_t)frames;
    if (hipMalloc(&d->speed_ws, bytes) != hipSuccess) {
        d->speed_ws = nullptr;
        mio::set_error("pcm_speed: workspace of %zu bytes failed", bytes);
        return MIO_ERR_OOM;
    }
    std::vector<float> w(mio::SP_N);  // periodic Hann, designed in float64
    for (int i = 0; i < mio::SP_N; ++i) w[i] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * i / mio::SP_N));
    MIO_HIP_CHECK(hipMemcpy(d->speed_ws, w.data(), sizeof(float) * mio::SP_N, hipMemcpyHostToDevice));
    d->speed_frames = frames;
    return MIO_OK;
}

int check_speed(float speed, const char *who) {
    MIO_REQUIRE(speed >= 0.5f && speed <= 2.0f, MIO_ERR_UNSUPPORTED,
                "%s: speed %g is not supported (0.5 to 2.0)", who, (double)speed);
    return MIO_OK;
}

}  // namespace

extern "C" int mio_hip_pcm_speed_reserve(mio_hip_device *d, int64_t n_max) {
    MIO_REQUIRE(d && n_max >= 0 && n_max <= kMaxSamples, MIO_ERR_INVALID, "pcm_speed_reserve: bad argument");
    int rc = mio::bind(d);
    if (rc) return rc;
    return ensure_ws(d, frames_of(out_len(n_max, 0.5f)));
}

extern "C" int mio_hip_pcm_speed(mio_hip_device *d, const float *const *in, const int64_t *n, int B, float speed,
                                 float *const *out, const int64_t *out_cap, int64_t *n_out,
                                 int32_t *const *offsets, void *stream) {
    MIO_REQUIRE(d && in && n && out && out_cap && n_out, MIO_ERR_INVALID, "pcm_speed: null argument");
    MIO_REQUIRE(B >= 1 && B <= mio::SP_MAX_B, MIO_ERR_INVALID, "pcm_speed: %d utterances (1 to %d)", B,
                mio::SP_MAX_B);
    int rc = check_speed(speed, "pcm_speed");
    if (rc) return rc;
    long long frames = 0, hops = 0;
    for (int b = 0; b < B; ++b) {
        MIO_REQUIRE(n[b] >= 0 && n[b] <= kMaxSamples && (in[b] || n[b] == 0), MIO_ERR_INVALID,
                    "pcm_speed: utterance %d: %lld samples%s", b, (long long)n[b], in[b] ? "" : " at a null pointer");
        const long long no = out_len(n[b], speed);
        MIO_REQUIRE(out_cap[b] >= no && (out[b] || no == 0), MIO_ERR_INVALID,
                    "pcm_speed: utterance %d: %lld outputs for a buffer of %lld", b, no, (long long)out_cap[b]);
        frames = std::max(frames, frames_of(no));
        hops = std::max(hops, frames_of(no) - 1);
    }
    if ((rc = mio::bind(d)) || (rc = ensure_ws(d, frames))) return rc;
    mio::SpArgs a{};
    a.window = static_cast<const float *>(d->speed_ws);
    a.speed = speed, a.B = B;
    int *rows = reinterpret_cast<int *>(static_cast<float *>(d->speed_ws) + mio::SP_N);
    for (int b = 0; b < B; ++b) {
        mio::SpUtt &u = a.u[b];
        u.in = in[b], u.out = out[b], u.n = n[b];
        u.n_out = n_out[b] = out_len(n[b], speed);
        u.frames = (int)frames_of(u.n_out);
        u.ws_off = rows + (size_t)b * (size_t)d->speed_frames;
        u.user_off = offsets ? offsets[b] : nullptr;
    }
    hipStream_t s = mio::pick_stream(d, stream);
    if ((rc = mio::speed_search_launch(a, s))) return rc;
    return mio::speed_ola_launch(a, hops, s);
}
