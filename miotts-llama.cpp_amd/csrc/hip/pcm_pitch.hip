// Pitch in the PCM epilogue: the resampling half, an arbitrary-ratio windowed-sinc interpolator.
// The operation is fixed in include/mio_hip.h ("pitch"); this file is the one place its kernel
// lives. Output j sits at input position t_j = (double)j (double)r (pitch_pos), i_j = floor(t_j),
// f_j = t_j - i_j, and
//   y[j] = c sum_k x[i_j + k] h(c (k - f_j)),  k = -K + 1 .. K,  K = ceil(Z / c),  c = min(1, 1/r),
// h the linear interpolation of the prototype table (Q points per zero crossing, 0 from Z on).
//
// k_pitch. Every output has a fractional phase of its own (r is irrational), so there is no phase
// table to share and no coefficient matrix for an MFMA: the coefficient is interpolated per tap.
// A workgroup of 256 lanes owns tiles of 2048 consecutive outputs (tiles blockIdx.x, + gridDim.x,
// ... of utterance blockIdx.y) and holds in LDS
//   * the prototype table, 8196 floats (32.0 KB), staged once per workgroup with 16-byte loads;
//   * the tile's input span x[i_first - K + 1, i_last + K], at most 2 * 2048 + 64 + 3 floats
//     (16.3 KB), loaded per tile with 16-byte loads from a 16-byte aligned address at or below its
//     first input (scalar and zero-filled only where a quad crosses [0, n)).
// 48.3 KB together: three workgroups fit a compute unit's 160 KB.
//   Lanes. Lane l forms outputs l, l + 256, ... of the tile, four at a time: four independent f32
// FMA chains per lane, each in ascending k, hide the LDS latency of one another. At one tap a
// wave's 64 span reads lie r words apart: consecutive banks for r near 1, pairs on one word (a
// broadcast) for r = 0.5; at r = 2 they are 2 apart over 128 words, and the span's words swap
// within their pairs in every other block of 64 (pt_swz), which puts those blocks' reads on the odd
// banks. The two table words of a tap are neighbours, read as one 8-byte pair; which banks a wave's
// 64 pairs touch is decided by the phases f_j alone ("Pitch", counts them).
//   The table position is formed in float64 exactly as the definition writes it, c (k - f_j), so
// the kernel and the float64 reference pick the same two entries; the interpolation between them
// and the sum are f32.
#include "common.h"
#include "pcm_pitch.h"

#pragma clang fp contract(off)

namespace mio {
namespace {

__global__ __launch_bounds__(PT_NT) void k_pitch(PtArgs a) {
    static_assert(PT_TILE % (PT_NT * PT_GROUP) == 0 && PT_SPAN % 4 == 0, "the lane layout below");
    __shared__ float4 tab4[PT_TAB_WORDS / 4];
    __shared__ float xs[PT_SPAN];
    const PtUtt &u = a.u[blockIdx.y];
    const int tid = threadIdx.x;
    const long long n_tiles = (u.n_out + PT_TILE - 1) / PT_TILE;
    if ((long long)blockIdx.x >= n_tiles) return;

    const float4 *t4 = reinterpret_cast<const float4 *>(a.table);
    for (int i = tid; i < PT_TAB_WORDS / 4; i += PT_NT) tab4[i] = t4[i];
    const float *tab = reinterpret_cast<const float *>(tab4);

    const int K = a.K, T = 2 * K;
    const double cd = (double)a.c;
    // words from the last 16-byte boundary to in[0]: in + base below is 16-byte aligned
    const int mis = (int)((reinterpret_cast<unsigned long long>(u.in) >> 2) & 3);

    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long j0 = tile * PT_TILE;
        const long long left = u.n_out - j0;
        const int cnt = left < PT_TILE ? (int)left : PT_TILE;
        const long long i_first = (long long)__builtin_floor(pitch_pos(j0, a.r));
        const long long i_last = (long long)__builtin_floor(pitch_pos(j0 + cnt - 1, a.r));
        const long long base = ((i_first - K + 1 + mis) & ~3LL) - mis;
        const int span = (int)(i_last + K - base) + 1;
        if (span > PT_SPAN) return;  // not reached for 0.5 <= r <= 2: nothing is read past the span
        __syncthreads();  // the previous tile's reads of xs are done
        for (int q = tid; 4 * q < span; q += PT_NT) {
            const long long e = base + 4 * q;
            float4 v;
            if (e >= 0 && e + 3 < u.n) {
                v = *reinterpret_cast<const float4 *>(u.in + e);
            } else {
                v.x = e >= 0 && e < u.n ? u.in[e] : 0.0f;
                v.y = e + 1 >= 0 && e + 1 < u.n ? u.in[e + 1] : 0.0f;
                v.z = e + 2 >= 0 && e + 2 < u.n ? u.in[e + 2] : 0.0f;
                v.w = e + 3 >= 0 && e + 3 < u.n ? u.in[e + 3] : 0.0f;
            }
            const int w = 4 * q, sw = (w >> 6) & 1;  // pt_swz of the quad's four words
            xs[w + sw] = v.x, xs[w + 1 - sw] = v.y, xs[w + 2 + sw] = v.z, xs[w + 3 - sw] = v.w;
        }
        __syncthreads();  // the table (first tile) and the span are staged

        for (int g = 0; g < PT_TILE / PT_NT && g * PT_NT < cnt; g += PT_GROUP) {
            double f[PT_GROUP];
            int loc[PT_GROUP];
            float acc[PT_GROUP];
#pragma unroll
            for (int e = 0; e < PT_GROUP; ++e) {  // a lane past the tile's end repeats its last output
                const int jj = (g + e) * PT_NT + tid;
                const double t = pitch_pos(j0 + (jj < cnt ? jj : cnt - 1), a.r);
                const double fl = __builtin_floor(t);
                f[e] = t - fl;
                loc[e] = (int)((long long)fl - base) - K + 1;
                acc[e] = 0.0f;
            }
            for (int m = 0; m < T; ++m) {
                const double kd = (double)(m - K + 1);
#pragma unroll
                for (int e = 0; e < PT_GROUP; ++e) {
                    const double p = __builtin_fabs(cd * (kd - f[e])) * (double)PT_Q;
                    const int ip = (int)p;  // p < (K + 1) Q
                    const float fr = (float)(p - (double)ip);
                    const int idx = ip < PT_Z * PT_Q - 1 ? ip : PT_Z * PT_Q - 1;
                    const float t0 = tab[idx], t1 = tab[idx + 1];
                    const float h = ip < PT_Z * PT_Q ? __builtin_fmaf(fr, t1 - t0, t0) : 0.0f;
                    acc[e] = __builtin_fmaf(xs[pt_swz(loc[e] + m)], h, acc[e]);
                }
            }
#pragma unroll
            for (int e = 0; e < PT_GROUP; ++e) {
                const int jj = (g + e) * PT_NT + tid;
                if (jj < cnt) u.out[j0 + jj] = a.c * acc[e];
            }
        }
    }
}

}  // namespace

int pitch_launch(const PtArgs &a, int tiles_x, hipStream_t s) {
    if (tiles_x <= 0) return MIO_OK;
    MIO_REQUIRE(a.B >= 1 && a.B <= PT_MAX_B && a.r >= 0.5f && a.r <= 2.0f && a.K >= PT_Z && 2 * a.K <= PT_MAX_TAPS,
                MIO_ERR_INVALID, "pitch: launch with ratio %g, %d taps a side, %d utterances", (double)a.r, a.K, a.B);
    hipLaunchKernelGGL(k_pitch, dim3((unsigned)tiles_x, a.B), dim3(PT_NT), 0, s, a);
    MIO_HIP_CHECK(hipGetLastError());
    return MIO_OK;
}

}  // namespace mio
