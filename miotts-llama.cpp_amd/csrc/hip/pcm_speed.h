// Launch interface of the WSOLA time-scale kernels (pcm_speed.hip): the lag search and the
// overlap-add of mio_hip_pcm_speed (include/mio_hip.h, "speaking rate").
#pragma once

#include <hip/hip_runtime.h>

namespace mio {

constexpr int SP_N = 1024;      // frame length
constexpr int SP_HS = 512;      // synthesis hop
constexpr int SP_D = 512;       // lags searched: [-D, D)
constexpr int SP_MAX_B = 16;    // utterances of one call
constexpr int SP_SPAN = SP_N + 2 * SP_D;  // inputs one frame's search reads
constexpr int SP_NT = 256;      // threads of a workgroup, both kernels
constexpr int SP_LPT = 2 * SP_D / SP_NT;  // consecutive lags one lane scores (its register window)

// one utterance of a call; passed by value in the kernel arguments (no descriptor copy)
struct SpUtt {
    const float *in;     // n samples at the codec's rate
    float *out;          // n_out samples
    int *ws_off;         // offsets[frames] in the workspace (the overlap-add reads these)
    int *user_off;       // the caller's copy, or null
    long long n, n_out;
    int frames;          // ceil(n_out / Hs) + 1
};

struct SpArgs {
    SpUtt u[SP_MAX_B];
    const float *window;  // w[0 .. N) (float64 design, rounded to f32)
    float speed;
    int B;
};

// nominal start of frame m: floor((m - 1) Hs (double)s + 0.5), the one expression host, device
// and reference share (no contraction: the product is rounded before the sum)
__host__ __device__ inline long long speed_frame_start(int m, float speed) {
#pragma clang fp contract(off)
    const double t = (double)((long long)(m - 1) * SP_HS) * (double)speed;
    return (long long)__builtin_floor(t + 0.5);
}

// the search: B persistent workgroups, one per utterance, each walking its frames
int speed_search_launch(const SpArgs &a, hipStream_t s);
// the overlap-add: one launch over every hop of every utterance (max_hops = the longest one's)
int speed_ola_launch(const SpArgs &a, long long max_hops, hipStream_t s);

}  // namespace mio
