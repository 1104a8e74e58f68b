// Speaking rate in the PCM epilogue: time-scale modification by WSOLA (waveform-similarity
// overlap-add) on the iSTFT's floats. The operation is fixed in include/mio_hip.h ("speaking
// rate"); this file is the one place its two kernels live.
//
// k_speed_search. The chain over the frames is sequential only through one integer, the previous
// frame's offset, so ONE persistent workgroup of 256 lanes walks an utterance's frames and the grid
// holds one workgroup per utterance: a batch's chains run side by side on as many compute units.
// Per frame m the LDS holds the input span x[p_m - D, p_m + D + N) (2048 floats, 8 KB) and the
// template t = x[a_{m-1} + Hs, + N) (4 KB). Only the template depends on the previous offset, so
// the NEXT frame's span is fetched from HBM into registers before the scoring loop (8 loads per
// lane, in flight while the loop runs) and stored to the second span buffer after it.
//   Scoring. Lane l owns the four neighbouring lags 4l - D .. 4l - D + 3, which share all but
// three of their inputs: for the four taps i = 4k .. 4k + 3 they need span words 4l + 4k ..
// 4l + 4k + 6, i.e. the aligned float4 at l + k and three words of the one at l + k + 1. The lane
// keeps that seven-word window in registers and slides it by one float4 per step, so a step costs
// ONE 16-byte span read (lanes read consecutive float4s: no bank conflict) and ONE 16-byte
// template read (every lane the same address: a broadcast) for 32 multiply-adds (4 lags x 4 taps
// x {dot, energy}), where one lag per lane would read a span word per multiply-add pair. Each
// lag's dot product and energy are single f32 FMA chains in the order i = 0 .. N - 1.
//   A sliding correlation has no matrix form worth its set-up: the Toeplitz operand an MFMA would
// need repeats every span word N times, so the instruction would spend its width on copies; the
// loop is bound by the FMA rate of the one compute unit the chain lives on.
//   Argmax with the tie rule (largest score, then smallest |lag|, then the smaller lag): in the
// lane, across the wave by shuffles, across the four waves through 4 LDS slots which every lane
// then reduces the same way, so the winner needs no second broadcast.
//
// k_speed_ola. One workgroup per hop of Hs outputs and utterance (grid hops x B, one launch for the
// batch): outputs of hop q lie in frames q and q + 1 only, so the two frame starts are uniform
// over the workgroup and each lane forms two outputs from two windowed reads each:
//   y = w[r + Hs] x1 + w[r] x2,  x1 = x[a_q + Hs + r], x2 = x[a_{q+1} + r],
// evaluated as fma(w[r + Hs], x1 - x2, x2) (w[r] = 1 - w[r + Hs] to half an ulp of f32): where both
// frames read the same sample (speed 1, or equal alignment) the output is that sample, bit for bit.
#include "common.h"
#include "pcm_speed.h"

#pragma clang fp contract(off)

namespace mio {
namespace {

// x[i], 0 outside [0, n); n >= 1. The load itself is unconditional, from the clamped index, so a
// lane's loads issue back to back instead of one branch and one wait each.
__device__ __forceinline__ float x_at(const float *x, long long n, long long i) {
    const long long c = i < 0 ? 0 : (i < n ? i : n - 1);
    const float v = x[c];
    return c == i ? v : 0.0f;
}

// the tie rule: is (c1, d1) to be preferred over (c2, d2)?
__device__ __forceinline__ bool better(float c1, int d1, float c2, int d2) {
    if (c1 != c2) return c1 > c2;
    const int a1 = d1 < 0 ? -d1 : d1, a2 = d2 < 0 ? -d2 : d2;
    return a1 != a2 ? a1 < a2 : d1 < d2;
}

__global__ __launch_bounds__(SP_NT) void k_speed_search(SpArgs a) {
    static_assert(SP_LPT == 4 && SP_SPAN == 8 * SP_NT && SP_N == 4 * SP_NT, "the lane layout below");
    // one float4 more than is used: the loop below reads one step ahead, the last step past the data
    __shared__ float4 span4[2][SP_SPAN / 4 + 1];
    __shared__ float4 tmpl4[SP_N / 4 + 1];
    __shared__ float red_c[SP_NT / 64];
    __shared__ int red_d[SP_NT / 64];
    const SpUtt &u = a.u[blockIdx.x];
    const int tid = threadIdx.x;
    const float *x = u.in;
    const long long n = u.n;

    if (tid == 0) {
        u.ws_off[0] = 0;
        if (u.user_off) u.user_off[0] = 0;
    }
    if (u.frames < 2) return;

    long long a_prev = speed_frame_start(0, a.speed);
    long long p = speed_frame_start(1, a.speed);
    {
        float *s0 = reinterpret_cast<float *>(span4[0]);
#pragma unroll
        for (int j = 0; j < 8; ++j) s0[tid + SP_NT * j] = x_at(x, n, p - SP_D + tid + SP_NT * j);
    }

    for (int m = 1; m < u.frames; ++m) {
        const int cur = (m - 1) & 1;
        float *tm = reinterpret_cast<float *>(tmpl4);
#pragma unroll
        for (int j = 0; j < 4; ++j) tm[tid + SP_NT * j] = x_at(x, n, a_prev + SP_HS + tid + SP_NT * j);
        // the next frame's span: loads issued here, stored after the scoring loop
        const bool more = m + 1 < u.frames;
        const long long p_next = more ? speed_frame_start(m + 1, a.speed) : 0;
        float pre[8];
        if (more) {
#pragma unroll
            for (int j = 0; j < 8; ++j) pre[j] = x_at(x, n, p_next - SP_D + tid + SP_NT * j);
        }
        __syncthreads();  // template and span[cur] are staged

        const float4 *S4 = span4[cur];
        float dot[4] = {0.0f, 0.0f, 0.0f, 0.0f}, en[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        // the next step's two reads are issued before this step's 32 multiply-adds: with one wave
        // per SIMD nothing else hides the LDS latency
        float4 w0 = S4[tid], w1 = S4[tid + 1], t4 = tmpl4[0];
#pragma unroll 2
        for (int k = 0; k < SP_N / 4; ++k) {
            const float4 w2 = S4[tid + k + 2];
            const float4 t4n = tmpl4[k + 1];
            const float win[7] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z};
            const float t[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float s = win[r + i];
                    dot[r] = __builtin_fmaf(t[i], s, dot[r]);
                    en[r] = __builtin_fmaf(s, s, en[r]);
                }
            }
            w0 = w1, w1 = w2, t4 = t4n;
        }

        float best_c = dot[0] / sqrtf(en[0] + 1e-12f);
        int best_d = 4 * tid - SP_D;
#pragma unroll
        for (int r = 1; r < 4; ++r) {
            const float c = dot[r] / sqrtf(en[r] + 1e-12f);
            const int d = 4 * tid + r - SP_D;
            if (better(c, d, best_c, best_d)) best_c = c, best_d = d;
        }
        for (int o = 32; o > 0; o >>= 1) {
            const float c = __shfl_xor(best_c, o);
            const int d = __shfl_xor(best_d, o);
            if (better(c, d, best_c, best_d)) best_c = c, best_d = d;
        }
        if ((tid & 63) == 0) red_c[tid >> 6] = best_c, red_d[tid >> 6] = best_d;
        if (more) {  // span[cur ^ 1] was last read in the previous frame's loop, two barriers ago
            float *sn = reinterpret_cast<float *>(span4[cur ^ 1]);
#pragma unroll
            for (int j = 0; j < 8; ++j) sn[tid + SP_NT * j] = pre[j];
        }
        __syncthreads();  // the waves' winners, the next span; every lane is past its reads of the template
        best_c = red_c[0], best_d = red_d[0];
#pragma unroll
        for (int w = 1; w < SP_NT / 64; ++w)
            if (better(red_c[w], red_d[w], best_c, best_d)) best_c = red_c[w], best_d = red_d[w];
        if (tid == 0) {
            u.ws_off[m] = best_d;
            if (u.user_off) u.user_off[m] = best_d;
        }
        a_prev = p + best_d;
        p = p_next;
        // the next frame writes red_c / red_d only after its own first barrier
    }
}

__global__ __launch_bounds__(SP_NT) void k_speed_ola(SpArgs a) {
    const SpUtt &u = a.u[blockIdx.y];
    const long long q = blockIdx.x, j0 = q * SP_HS;
    if (j0 >= u.n_out) return;  // then q + 1 <= frames - 1 = ceil(n_out / Hs)
    const long long a1 = speed_frame_start((int)q, a.speed) + u.ws_off[q] + SP_HS;
    const long long a2 = speed_frame_start((int)q + 1, a.speed) + u.ws_off[q + 1];
    for (int r = threadIdx.x; r < SP_HS; r += SP_NT) {
        if (j0 + r >= u.n_out) break;
        const float x1 = x_at(u.in, u.n, a1 + r), x2 = x_at(u.in, u.n, a2 + r);
        u.out[j0 + r] = x1 == x2 ? x2 : __builtin_fmaf(a.window[r + SP_HS], x1 - x2, x2);
    }
}

}  // namespace

int speed_search_launch(const SpArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(k_speed_search, dim3(a.B), dim3(SP_NT), 0, s, a);
    MIO_HIP_CHECK(hipGetLastError());
    return MIO_OK;
}

int speed_ola_launch(const SpArgs &a, long long max_hops, hipStream_t s) {
    if (max_hops <= 0) return MIO_OK;
    hipLaunchKernelGGL(k_speed_ola, dim3((unsigned)max_hops, a.B), dim3(SP_NT), 0, s, a);
    MIO_HIP_CHECK(hipGetLastError());
    return MIO_OK;
}

}  // namespace mio
