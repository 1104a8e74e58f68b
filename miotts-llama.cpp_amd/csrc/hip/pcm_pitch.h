// Launch interface of the arbitrary-ratio sinc interpolator (pcm_pitch.hip): the resampling half
// of mio_hip_pcm_pitch (include/mio_hip.h, "pitch").
#pragma once

#include <hip/hip_runtime.h>

namespace mio {

constexpr int PT_Z = 16;                   // zero crossings of the prototype per side
constexpr int PT_Q = 512;                  // table points per zero crossing
constexpr int PT_TAB = PT_Z * PT_Q + 1;    // table entries: h(i / Q), i = 0 .. Z Q
constexpr int PT_TAB_WORDS = (PT_TAB + 3) / 4 * 4;  // as stored: zero-padded to whole float4s
constexpr double PT_BETA = 0.1102 * (80.0 - 8.7);   // Kaiser beta of an 80 dB design (7.857)
constexpr int PT_MAX_B = 16;               // utterances of one call
constexpr int PT_NT = 256;                 // threads of a workgroup
constexpr int PT_TILE = 2048;              // consecutive outputs of one tile
constexpr int PT_GROUP = 4;                // outputs a lane carries through the tap loop at once
constexpr int PT_MAX_TAPS = 4 * PT_Z;      // 2 ceil(Z / c) at the largest ratio, 2
// inputs a tile can reach: floor-to-floor distance of its first and last position (< 2 TILE), the
// taps, and up to 3 more in front for the 16-byte alignment of the loads
constexpr int PT_SPAN = 2 * PT_TILE + PT_MAX_TAPS + 4;
// where span word w lives in LDS: words of every other block of 64 swap within their pairs. At
// ratio 2 a wave's 64 reads of one tap lie 2 words apart over two or three such blocks, and the
// swap puts the odd blocks' reads on the odd banks: 64 banks, whatever the alignment.
__host__ __device__ inline int pt_swz(int w) { return w ^ ((w >> 6) & 1); }

// one utterance of a call; passed by value in the kernel arguments (no descriptor copy)
struct PtUtt {
    const float *in;   // n samples
    float *out;        // n_out samples
    long long n, n_out;
};

struct PtArgs {
    PtUtt u[PT_MAX_B];
    const float *table;  // PT_TAB_WORDS floats
    float r;             // input step per output
    float c;             // cutoff and gain, min(1, 1 / r) in f32
    int K;               // ceil(Z / c): taps k = -K + 1 .. K
    int B;
};

// position of output j in the input: (double)j (double)r, the one expression host, device and
// reference share (one rounded product, no contraction)
__host__ __device__ inline double pitch_pos(long long j, float r) {
#pragma clang fp contract(off)
    return (double)j * (double)r;
}

// one launch for the batch: grid (tiles_x, B); a workgroup walks tiles blockIdx.x, + gridDim.x, ...
int pitch_launch(const PtArgs &a, int tiles_x, hipStream_t s);

}  // namespace mio
