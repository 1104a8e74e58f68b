// Rational resampler of the PCM epilogue: output at L / M times the input rate through a
// Kaiser-windowed sinc held as a phase table (designed in csrc/capi/resample_capi.cpp).
//
// The one place the indexing is fixed. With b(n) = floor(n M / L) and phi(n) = n M mod L,
//   y[n] = sum_{t < P} x[b(n) - P/2 + 1 + t] * c[phi(n)][P - 1 - t],   c[phi][j] = h[j L + phi],
// x = 0 outside the signal, n and the x index counted from the start of the stream. The table
// the kernel reads is already in tap order: row phi holds c[phi][P - 1 - t] at column t.
//
// One workgroup of nt threads per tile of nt consecutive outputs; a workgroup walks tiles
// blockIdx.x, blockIdx.x + gridDim.x, ... so the phase table is staged into LDS once per
// workgroup (16-byte loads), not once per tile. Per tile the input span b(first) - P/2 + 1 ..
// b(last) + P/2 goes to LDS, each sample multiplied by the input gain as it is loaded
// (mio_hip_pcm_normalize's expression), from the previous call's P - 1 kept samples where the
// index lies before this call's input and as 0 outside the stream. Every thread then forms its
// output as ONE chain acc = fma(x_t, c_t, acc), t = 0 .. P - 1, from acc = 0: the order depends
// on nothing but t, so tiles, grids and the cut of the stream into calls give the same bits.
//
// LDS reads of a wave at tap t: lane j reads table word row(j) * cs + t with row(j) = (row(0) +
// j (M mod L)) mod L, and x word b(n0 + j) - b(n0) + t. The row stride cs >= P is chosen on the
// host so that the 64 rows of a wave fall on as many of the 64 banks as possible (DESIGN 4,
// "Output rate"); the x reads of an up-sampling ratio share words (broadcast), those of a
// down-sampling one spread over ceil(64 M / L) consecutive words.
#include "common.h"
#include "pcm_resample.h"

#include <type_traits>

#pragma clang fp contract(off)

namespace mio {
namespace {

__device__ __forceinline__ float max_keep(float peak, float a) { return peak < a ? a : peak; }

// input number `a` of the stream as this call sees it (gain applied); hist holds loaded values
__device__ __forceinline__ float load_x(const RsArgs &a, long long i, bool scale, float gain) {
    if (i < 0 || i >= a.seen + a.n_in) return 0.0f;
    if (i < a.seen) {
        const long long k = i - (a.seen - (a.P - 1));
        return k < 0 ? 0.0f : a.hist[k];
    }
    float v = a.in[i - a.seen];
    if (scale) v = v * gain;
    return v;
}

template <class OutT>
__global__ __launch_bounds__(RS_NT_MAX) void k_resample(RsArgs a) {
    extern __shared__ float4 lds4[];
    __shared__ float red[RS_NT_MAX / 64];
    __shared__ float gain_s;
    __shared__ int scale_s;
    float *tab = reinterpret_cast<float *>(lds4);
    float *xs = tab + a.tab_words;
    const int nt = blockDim.x;

    float gain = a.gain;
    bool scale = a.gain != 1.0f;
    if (a.part) {  // the normalising gain from the peak partials, as k_finish forms it
        float m = 0.0f;
        for (int i = threadIdx.x; i < a.n_parts; i += nt) m = max_keep(m, a.part[i]);
        for (int o = 32; o > 0; o >>= 1) m = max_keep(m, __shfl_xor(m, o));
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
        __syncthreads();
        if (threadIdx.x == 0) {
            float r = red[0];
            for (int w = 1; w < nt / 64; ++w) r = max_keep(r, red[w]);
            if (a.peak_out && blockIdx.x == 0) *a.peak_out = r;
            scale_s = r > 1e-8f;
            gain_s = 0.95f / r;
        }
        __syncthreads();
        scale = scale_s != 0;
        gain = gain_s;
    }

    const float4 *t4 = reinterpret_cast<const float4 *>(a.table);
    for (int i = threadIdx.x; i < a.tab_words / 4; i += nt) lds4[i] = t4[i];

    // the last P - 1 inputs seen, for the next call (the other buffer of a pair: no workgroup
    // of this launch reads what this one writes)
    if (a.hist_next && blockIdx.x == 0) {
        const long long first = a.seen + a.n_in - (a.P - 1);
        for (int i = threadIdx.x; i < a.P - 1; i += nt) a.hist_next[i] = load_x(a, first + i, scale, gain);
    }

    const long long n_tiles = (a.n_out + nt - 1) / nt;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long n0 = a.out0 + tile * nt;
        const long long left = a.out0 + a.n_out - n0;
        const int cnt = left < nt ? (int)left : nt;
        const long long b0 = (n0 * a.M) / a.L;
        const int span = (int)(((n0 + cnt - 1) * a.M) / a.L - b0) + a.P;
        const long long x0 = b0 - a.P / 2 + 1;
        __syncthreads();  // the table is staged; the previous tile's reads of xs are done
        for (int i = threadIdx.x; i < span; i += nt) xs[i] = load_x(a, x0 + i, scale, gain);
        __syncthreads();
        if ((int)threadIdx.x < cnt) {
            const long long n = n0 + threadIdx.x;
            const long long q = n * a.M;
            const long long b = q / a.L;
            const float *c = tab + (int)(q - b * a.L) * a.cs;
            const float *x = xs + (int)(b - b0);
            float acc = 0.0f;
#pragma unroll 4
            for (int t = 0; t < a.P; ++t) acc = __builtin_fmaf(x[t], c[t], acc);
            OutT *out = static_cast<OutT *>(a.out);
            if constexpr (std::is_same_v<OutT, short>)
                out[n - a.out0] = pcm16_sample(acc);
            else
                out[n - a.out0] = acc;
        }
    }
}

}  // namespace

int resample_prepare() {
    MIO_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_resample<float>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, RS_LDS_MAX - RS_LDS_STATIC));
    MIO_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_resample<short>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, RS_LDS_MAX - RS_LDS_STATIC));
    return MIO_OK;
}

int resample_launch(const RsArgs &a, bool pcm16, int grid, int nt, hipStream_t s) {
    const size_t lds = resample_lds_bytes(a.tab_words, a.L, a.M, a.P, nt);
    MIO_REQUIRE(grid >= 1 && nt >= 64 && nt <= RS_NT_MAX && nt % 64 == 0 && a.tab_words % 4 == 0 &&
                    lds + RS_LDS_STATIC <= (size_t)RS_LDS_MAX,
                MIO_ERR_INVALID, "resample: launch of %d x %d with %zu bytes of LDS", grid, nt, lds);
    if (pcm16)
        hipLaunchKernelGGL(k_resample<short>, dim3(grid), dim3(nt), lds, s, a);
    else
        hipLaunchKernelGGL(k_resample<float>, dim3(grid), dim3(nt), lds, s, a);
    MIO_HIP_CHECK(hipGetLastError());
    return MIO_OK;
}

}  // namespace mio
