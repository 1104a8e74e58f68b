// Launch interface of the rational resampler kernel (pcm_resample.hip); the handle, the filter
// design and the C-ABI are in csrc/capi/resample_capi.cpp.
#pragma once

#include <hip/hip_runtime.h>

namespace mio {

constexpr int RS_NT_MAX = 1024;     // threads (= outputs of one tile) per workgroup, at most
constexpr int RS_LDS_MAX = 160 * 1024;
constexpr int RS_LDS_STATIC = 1024;  // kept for the kernel's static LDS (the gain's reduction)
constexpr int RS_MAX_PARTS = 1024;  // peak partials of the normalising pass (pcm_finish.hip)

struct RsArgs {
    const float *in;      // this call's n_in samples; in[0] is input number `seen` of the stream
    long long n_in, seen;
    const float *hist;    // inputs [seen - (P - 1), seen) as they were loaded (gain applied)
    float *hist_next;     // receives inputs [seen + n_in - (P - 1), seen + n_in); null: not kept
    long long out0, n_out;  // outputs [out0, out0 + n_out) of the stream
    const float *table;   // LDS image of the phase table: row phi at phi * cs, tap order
    int tab_words;        // its size in floats, a multiple of 4
    int L, M, P, cs;
    // input gain: `gain` (host value), or, with part != null, 0.95 / max(part[0 .. n_parts))
    // where that maximum is > 1e-8 (mio_hip_pcm_normalize's rule), the maximum to *peak_out
    float gain;
    const float *part;
    int n_parts;
    float *peak_out;
    void *out;            // float or int16_t [n_out]
};

// Peak partials of samples[0 .. n) (16-byte aligned) into part[0 .. *parts), *parts <= RS_MAX_PARTS:
// the first pass of mio_hip_pcm_finish (pcm_finish.hip).
int pcm_peak_launch(const float *samples, long long n, float *part, int *parts, hipStream_t s);

// hipFuncAttributeMaxDynamicSharedMemorySize on both instantiations, for the current device
int resample_prepare();
// one launch: `grid` workgroups of nt threads (a multiple of 64) walk the tiles of nt outputs
int resample_launch(const RsArgs &a, bool pcm16, int grid, int nt, hipStream_t s);
// dynamic LDS of a launch: the table and the input span of one tile of nt outputs
inline size_t resample_lds_bytes(int tab_words, int L, int M, int P, int nt) {
    return 4 * ((size_t)tab_words + (size_t)(((long long)(nt - 1) * M) / L + 1 + P));
}

}  // namespace mio
