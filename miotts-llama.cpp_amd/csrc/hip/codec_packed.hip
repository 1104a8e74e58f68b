// Packed MioCodec decode for gfx950 (CDNA4): B <= 16 utterances of different lengths and
// voices concatenated along the row axis into one activation [sum S_b][C], run through one
// launch set. The row-independent GEMMs, the embedding and the k = stride wave_upsample ConvT
// run on the packed rows through the kernels of codec_kernels.hip unchanged; this file holds
// the kernels that must know where an utterance ends.
//
// Segment table: B + 1 row offsets per stage resolution, in the workspace (`off` below). No
// row -> segment map: a kernel finds a row's segment by a search over the <= 17 offsets, which
// are wave-uniform loads (the table stays in the scalar cache), and only where a tile can
// touch more than one segment; a tile inside one segment does the search twice (its first and
// last row) and nothing per row. A map would cost a 4-byte read per row per kernel and one
// more buffer per resolution to fill.
//
//  * seg_gemm_kernel      : f32 GEMM on v_mfma_f32_32x32x2_f32, 64 x 64 tiles, whose A operand
//                           is a tap window clipped to the row's segment (ConvTranspose with
//                           kernel > stride: a tap that would read a neighbour reads zero) and
//                           whose epilogue is per segment: AdaLN gate[segment][n], or the ConvT
//                           remap + trim + Snake into the segment's rows of the next stage.
//  * seg_conv_f16_kernel  : Conv1d as implicit GEMM on v_mfma_f32_32x32x16_f16 with the "same"
//                           zero padding at every segment edge. A tile inside one segment
//                           points its buffer descriptor at that segment (the hardware range
//                           check is the padding, as in the single decode: no per-row work); a
//                           straddling tile keeps two bounds per staged row in registers.
//  * seg_gn_*             : GroupNorm statistics per (segment, group); slices never span two
//                           segments and a segment is cut exactly as the single decode cuts it,
//                           so its sums run in an order that does not depend on its neighbours.
//  * seg_band_attention   : a workgroup never spans two segments; band and LDS key window are
//                           clipped to the segment, RoPE by the position inside it.
//  * seg_rownorm_kernel   : AdaLN modulate with shift / scale[segment].
//  * cond_gemv_batch      : the conditioning vectors of all B voices, W read once.
#include "codec_kernels.h"

#include <algorithm>
#include <cmath>
#include <type_traits>

#pragma clang fp contract(off)

namespace mio {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float silu_f(float x) { return x / (1.0f + expf(-x)); }

__device__ __forceinline__ float snake_f(float v, float a, float b) {
    const float ax = v * a;
    const float s = sinf(ax);
    const float s2 = s * s;
    return v + s2 / b;
}

// segment of `row`: the last b with off[b] <= row (row < off[B])
__device__ __forceinline__ int seg_of(const int *off, int B, int row) {
    int b = 0;
    while (b + 1 < B && row >= off[b + 1]) ++b;
    return b;
}

// ---------------------------------------------------------------- segment-aware f32 GEMM
// 64 x 64 tile, 2 x 2 waves of 32 x 32. 32-deep stages: the next stage's operands are in
// flight in registers (buffer loads, out-of-range = 0) while the MFMAs read the current one from
// LDS; two LDS buffers, one barrier per stage.
// KG: the K-groups of the single decode's GEMM of these segments (gemm_f32_kernel: K-group q
// owns k in [32q, 32q + 32) of every 32 KG-deep stage, one exact f32 fma chain each, the chains
// added once in K-group order). Here the packed M fills the chip without splitting K over
// waves, so a wave keeps the KG chains as KG accumulators, 32-deep stage j feeding chain
// j mod KG, and adds them in the same order: every output is its single-decode value bit for
// bit. One launch covers a run of segments with the same KG (rows [m_begin, M)).
constexpr int SG_T = 64, SG_BK = 32, SG_LDK = SG_BK + 4;

template <int EPI, int KG>
__global__ __launch_bounds__(256) void seg_gemm_kernel(SegGemmArgs g) {
    constexpr int AV = SG_T * SG_BK / 4 / 256;  // float4 per thread per operand and stage
    __shared__ __attribute__((aligned(16))) float As[2][SG_T * SG_LDK];
    __shared__ __attribute__((aligned(16))) float Bs[2][SG_T * SG_LDK];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = g.m_begin + blockIdx.y * SG_T, n0 = blockIdx.x * SG_T;
    const int mlast = min(m0 + SG_T, g.M) - 1;
    // segments of the tile's first and last row: equal for a tile inside one segment
    const int bt0 = seg_of(g.m_off, g.nseg, m0), bt1 = seg_of(g.m_off, g.nseg, mlast);

    f32x16 accs[KG];
#pragma unroll
    for (int q = 0; q < KG; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) accs[q][r] = 0.0f;

    const auto ra_src = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(g.A), 0,
                                                          (int)((long)g.a_off[g.nseg] * g.a_seg * 4), 0x00020000);
    const auto rb_src = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(g.B), 0,
                                                          (int)((long)g.N * g.K * 4), 0x00020000);
    // per staged A row: element (m, k) of the tap window is A[a_base + k], inside the row's
    // segment exactly when a_lo <= a_base + k < a_hi (the single decode's [0, a_rows) mask,
    // per segment); a row past M has an empty range
    int a_base[AV], a_lo[AV], a_hi[AV], a_c[AV], b_off[AV], b_c[AV];
#pragma unroll
    for (int i = 0; i < AV; ++i) {
        const int e = tid + i * 256, m = m0 + e / (SG_BK / 4);
        a_c[i] = (e % (SG_BK / 4)) * 4;
        int b = bt0;
        while (b < bt1 && m >= g.m_off[b + 1]) ++b;
        const bool in = m < g.M;
        a_lo[i] = in ? g.a_off[b] * g.a_seg : 0;
        a_hi[i] = in ? g.a_off[b + 1] * g.a_seg : 0;
        a_base[i] = (g.a_off[b] + (m - g.m_off[b]) - (g.taps - 1)) * g.a_seg + a_c[i];
        const int n = n0 + e / (SG_BK / 4);
        b_c[i] = a_c[i];
        b_off[i] = (n * g.K + b_c[i]) * 4;
    }
    float4 ra[AV], rb[AV];
    auto load = [&](int k0) {
#pragma unroll
        for (int i = 0; i < AV; ++i) {
            const int idx = a_base[i] + k0;
            const bool ok = k0 + a_c[i] < g.K && idx >= a_lo[i] && idx < a_hi[i];
            ra[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(ra_src, ok ? idx * 4 : (int)0x80000000, 0, 0));
        }
#pragma unroll
        for (int i = 0; i < AV; ++i) {
            const int off = k0 + b_c[i] < g.K ? b_off[i] + k0 * 4 : (int)0x80000000;
            rb[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rb_src, off, 0, 0));
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < AV; ++i) {
            const int e = tid + i * 256, r = e / (SG_BK / 4);
            float4 v = ra[i];
            if (g.a_f16) {  // F16 weight: ggml rounds the activation to f16 (exact f32 products)
                v.x = (float)(_Float16)v.x, v.y = (float)(_Float16)v.y;
                v.z = (float)(_Float16)v.z, v.w = (float)(_Float16)v.w;
            }
            *reinterpret_cast<float4 *>(&As[buf][r * SG_LDK + a_c[i]]) = v;
            *reinterpret_cast<float4 *>(&Bs[buf][r * SG_LDK + b_c[i]]) = rb[i];
        }
    };
    auto compute = [&](int buf, f32x16 &acc) {
#pragma unroll
        for (int o = 0; o < SG_BK / 8; ++o) {
            const int kc = o * 8 + 4 * (lane >> 5);
            const float4 a = *reinterpret_cast<const float4 *>(&As[buf][(wm * 32 + (lane & 31)) * SG_LDK + kc]);
            const float4 b = *reinterpret_cast<const float4 *>(&Bs[buf][(wn * 32 + (lane & 31)) * SG_LDK + kc]);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
        }
    };

    // whole 32 KG-deep stages as the single decode runs them: blocks past K are zeros
    const int nk = (g.K + SG_BK * KG - 1) / (SG_BK * KG) * KG;
    load(0);
    store(0);
    __syncthreads();
    for (int kt = 0; kt < nk; kt += KG) {
#pragma unroll
        for (int q = 0; q < KG; ++q) {
            load((kt + q + 1) * SG_BK);
            compute((kt + q) & 1, accs[q]);
            store((kt + q + 1) & 1);
            __syncthreads();
        }
    }
    f32x16 acc = accs[0];
#pragma unroll
    for (int q = 1; q < KG; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = acc[r] + accs[q][r];

    // ---- epilogue (C layout: col = lane&31, row = (r&3) + 8(r>>2) + 4(lane>>5))
    const int col = n0 + wn * 32 + (lane & 31);
    if (col >= g.N) return;
    int rr = 0, co = col;
    float pb = 0.0f, pa = 0.0f, pa2 = 1.0f;
    if constexpr (EPI == EPI_CONVT_SNAKE) {
        rr = col / g.cout, co = col - rr * g.cout;
        pb = g.bias[co], pa = g.aux[co], pa2 = g.aux2[co];
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m >= g.M) continue;
        int b = bt0;
        while (b < bt1 && m >= g.m_off[b + 1]) ++b;
        const float v = acc[r];
        if constexpr (EPI == EPI_GATED) {
            float *o = g.C + (long)m * g.ldc + col;
            const float gh = v * g.aux[(long)b * g.aux_ld + col];
            *o = *o + gh;
        } else {
            const int orow = g.f * (m - g.m_off[b]) + rr - g.trim;
            if (orow >= 0 && orow < g.c_off[b + 1] - g.c_off[b])
                g.C[(long)(g.c_off[b] + orow) * g.ldc + co] = snake_f(v + pb, pa, pa2);
        }
    }
}

// ---------------------------------------------------------------- segment-aware conv1d f16
// Tile, stages and MFMA order of the single decode's conv (64 x 64, 128-deep, k ascending in
// 16-chunks), so a segment's outputs are its single-decode outputs.
constexpr int CV_BM = 64, CV_BN = 64, CV_BK = 128, CV_LD = CV_BK + 8;

// STRADDLE = false: the tile's rows and their taps lie in one segment [lo, hi): the descriptor
// covers that segment alone and the hardware range check is the zero padding.
// STRADDLE = true: the descriptor covers the packed array and every staged row carries its
// segment's element range.
template <bool STRADDLE>
__device__ __forceinline__ void seg_conv_body(const ConvArgs &c, const int *off, int B, int lo, int hi,
                                              _Float16 (*As)[CV_BM * CV_LD], _Float16 (*Bs)[CV_BN * CV_LD]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.y * CV_BM, n0 = blockIdx.x * CV_BN;
    const int K = c.taps * c.Cin;
    constexpr int NV = CV_BM * CV_BK / 8 / 256;  // 16 B chunks per thread per operand

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;

    const int row0 = STRADDLE ? 0 : lo;  // first row the descriptor covers
    const int rows = STRADDLE ? c.L : hi - lo;
    const auto xa_src = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16 *>(c.Xa + (long)row0 * c.Cin), 0,
                                                          (int)((long)rows * c.Cin * 2), 0x00020000);
    const auto w_src = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16 *>(c.B), 0,
                                                         (int)((long)c.Cout * K * 2), 0x00020000);
    int r_lo[NV], r_hi[NV];
    if constexpr (STRADDLE) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int m = m0 + (tid + i * 256) / (CV_BK / 8);
            const bool in = m < c.L;
            const int b = seg_of(off, B, in ? m : 0);
            r_lo[i] = in ? off[b] * c.Cin : 0;
            r_hi[i] = in ? off[b + 1] * c.Cin : 0;
        }
    }
    uint4 ra[NV], rb[NV];
    auto load = [&](int k0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int e = tid + i * 256, r = e / (CV_BK / 8), k = k0 + (e % (CV_BK / 8)) * 8;
            const int idx = (m0 + r - c.pad - row0) * c.Cin + k;
            bool ok = k < K;
            if constexpr (STRADDLE) ok = ok && idx >= r_lo[i] && idx < r_hi[i];
            ra[i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(xa_src, ok ? idx * 2 : (int)0x80000000, 0, 0));
        }
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int e = tid + i * 256, r = e / (CV_BK / 8), k = k0 + (e % (CV_BK / 8)) * 8;
            const int o = k < K ? ((n0 + r) * K + k) * 2 : (int)0x80000000;
            rb[i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(w_src, o, 0, 0));
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int e = tid + i * 256, r = e / (CV_BK / 8), c8 = (e % (CV_BK / 8)) * 8;
            *reinterpret_cast<uint4 *>(&As[buf][r * CV_LD + c8]) = ra[i];
            *reinterpret_cast<uint4 *>(&Bs[buf][r * CV_LD + c8]) = rb[i];
        }
    };
    auto compute = [&](int buf) {
#pragma unroll
        for (int ks = 0; ks < CV_BK; ks += 16) {
            const f16x8 a = *reinterpret_cast<const f16x8 *>(&As[buf][(wm * 32 + (lane & 31)) * CV_LD + ks + 8 * (lane >> 5)]);
            const f16x8 b = *reinterpret_cast<const f16x8 *>(&Bs[buf][(wn * 32 + (lane & 31)) * CV_LD + ks + 8 * (lane >> 5)]);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0);
        }
    };

    // epilogue operands (bias, residual) loaded before the K loop, off its critical path
    const int col = n0 + wn * 32 + (lane & 31), colc = min(col, c.Cout - 1);
    const float bias = c.bias[colc];
    float res[16];
    const float *rsrc = c.resid ? c.resid : c.bias;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = min(m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), c.L - 1);
        res[r] = rsrc[c.resid ? (long)row * c.Cout + colc : colc];
    }

    const int nk = (K + CV_BK - 1) / CV_BK;
    load(0);
    store(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        load((kt + 1) * CV_BK);
        compute(kt & 1);
        store((kt + 1) & 1);
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (row < c.L && col < c.Cout) {
            float v = acc[r] + bias;
            if (c.resid) v = v + res[r];
            c.Y[(long)row * c.Cout + col] = v;
        }
    }
}

__global__ __launch_bounds__(256) void seg_conv_f16_kernel(ConvArgs c, const int *off, int B) {
    __shared__ __attribute__((aligned(16))) _Float16 As[2][CV_BM * CV_LD];
    __shared__ __attribute__((aligned(16))) _Float16 Bs[2][CV_BN * CV_LD];
    const int m0 = blockIdx.y * CV_BM;
    // rows the tile reads: its own and the taps' reach, clipped to the packed array
    const int first = max(m0 - c.pad, 0), last = min(m0 + CV_BM - 1 + (c.taps - 1 - c.pad), c.L - 1);
    const int b0 = seg_of(off, B, first), b1 = seg_of(off, B, last);
    if (b0 == b1)
        seg_conv_body<false>(c, off, B, off[b0], off[b0 + 1], As, Bs);
    else
        seg_conv_body<true>(c, off, B, 0, 0, As, Bs);
}

// ---------------------------------------------------------------- row norm, AdaLN per segment
template <int CTRL, int ROWS = 0xF>
__device__ __forceinline__ double dpp_f64(double x) {
    const int2 v = __builtin_bit_cast(int2, x);
    const int lo = __builtin_amdgcn_update_dpp(0, v.x, CTRL, ROWS, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, v.y, CTRL, ROWS, 0xF, false);
    return __builtin_bit_cast(double, make_int2(lo, hi));
}
// sum over the 64 lanes in double, the total in every lane (the order of rownorm_kernel)
__device__ __forceinline__ double wave_sum_f64(double s) {
    s += dpp_f64<0xB1>(s);        // quad_perm [1,0,3,2]
    s += dpp_f64<0x4E>(s);        // quad_perm [2,3,0,1]
    s += dpp_f64<0x141>(s);       // row_half_mirror
    s += dpp_f64<0x140>(s);       // row_mirror
    s += dpp_f64<0x142, 0xA>(s);  // row_bcast:15 -> rows 1, 3
    s += dpp_f64<0x143, 0xC>(s);  // row_bcast:31 -> rows 2, 3
    const int2 v = __builtin_bit_cast(int2, s);
    return __builtin_bit_cast(double, make_int2(__builtin_amdgcn_readlane(v.x, 63), __builtin_amdgcn_readlane(v.y, 63)));
}

// ggml_norm then y * (1 + scale[seg]) + shift[seg]; one wave per row, its segment found once
// per wave. shift / scale: [B][ld].
template <int NPL>
__global__ __launch_bounds__(256) void seg_rownorm_kernel(const float *x, float *y, int M, float eps,
                                                          const float *shift, const float *scale, int ld,
                                                          const int *off, int B) {
    constexpr int D = NPL * 64;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (row >= M) return;
    const int b = seg_of(off, B, row);
    const float *xr = x + (long)row * D, *sh = shift + (long)b * ld, *sc = scale + (long)b * ld;
    float v[NPL], pa[NPL], pb[NPL];
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
        v[i] = xr[i * 64 + lane];
        pa[i] = sh[i * 64 + lane];
        pb[i] = sc[i * 64 + lane];
    }
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < NPL; ++i) s += (double)v[i];
    s = wave_sum_f64(s);
    const float mean = (float)(s / D);
    double s2 = 0.0;
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
        v[i] = v[i] - mean;
        s2 += (double)(v[i] * v[i]);
    }
    s2 = wave_sum_f64(s2);
    const float variance = (float)(s2 / D);
    const float rs = 1.0f / sqrtf(variance + eps);
    float *yr = y + (long)row * D;
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
        float t = v[i] * rs;
        t = t * (1.0f + pb[i]);
        yr[i * 64 + lane] = t + pa[i];
    }
}

// ---------------------------------------------------------------- group norm per segment
// Grid (slices, B): workgroup (p, b) owns slice p of segment b. A segment of L rows is cut into
// P = ceil(L / rows) slices of rows = max(4, ceil(L / 128)) rows, the single decode's cut of an
// L-row sequence, and its partials live in part[b][p][g]; blocks past P leave. The slice sums
// (4 waves over rows r0 + w, r0 + w + 4, ..), their reduction (32 lanes per group, lane s takes
// slices s, s + 32, .., xor tree) and the double -> float steps follow gn_partial / gn_reduce of
// codec_kernels.hip, so (mean, rstd) of a segment are those of its single decode.
constexpr int SGN_P = 128;  // slices per segment at most

__device__ __forceinline__ int sgn_rows(int L) { return (L + 3) / 4 > SGN_P ? (L + SGN_P - 1) / SGN_P : 4; }

// out[g] = sum of the P slice partials part[p][g], g < G <= 64; 256 threads
__device__ __forceinline__ void sgn_reduce(const double *part, int P, int G, double *out) {
    const int t = threadIdx.x, s32 = t & 31;
    for (int g0 = 0; g0 < G; g0 += 8) {
        const int g = g0 + (t >> 5), gg = g < G ? g : 0;
        double sum = 0.0;
#pragma unroll
        for (int i = 0; i < SGN_P / 32; ++i)
            if (s32 + 32 * i < P) sum += part[(long)(s32 + 32 * i) * G + gg];
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) sum += __shfl_xor(sum, o);
        if (s32 == 0 && g < G) out[g] = sum;
    }
    __syncthreads();
}

// PASS 1: slice sums of x -> part1. PASS 2: the segment's means from part1, then slice sums of
// fl(fl(x - mean)^2) -> part2.
template <int PASS, int NJ>
__global__ __launch_bounds__(256) void seg_gn_partial_kernel(const float *x, const int *off, int C, int G, int cpg,
                                                             const double *part1, double *part_out) {
    __shared__ double red[64];
    __shared__ double wsum[4][64];
    const int b = blockIdx.y, p = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s0 = off[b], L = off[b + 1] - s0;
    const int rows = sgn_rows(L), P = (L + rows - 1) / rows;
    if (p >= P) return;
    const int r0 = s0 + p * rows, r1 = min(s0 + L, r0 + rows);
    const long n = (long)L * cpg;
    double acc[NJ];
    float mean[NJ];
    bool ok[NJ];
    int ch[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        ok[j] = j * 64 + lane < C;
        ch[j] = ok[j] ? j * 64 + lane : 0;
        acc[j] = 0.0;
        mean[j] = 0.0f;
    }
    if constexpr (PASS == 2) {
        sgn_reduce(part1 + (long)b * SGN_P * G, P, G, red);
#pragma unroll
        for (int j = 0; j < NJ; ++j) mean[j] = (float)(red[ch[j] / cpg] / (double)n);
    }
    for (int r = r0 + wave; r < r1; r += 4) {
        const float *xr = x + (long)r * C;
        float v[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) v[j] = xr[ch[j]];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const float d = v[j] - mean[j];
            acc[j] += ok[j] ? (double)(PASS == 1 ? v[j] : d * d) : 0.0;
        }
    }
    // a group is cpg consecutive lanes of one 64-channel chunk
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        double s = acc[j];
        for (int o = 1; o < cpg; o <<= 1) s += __shfl_xor(s, o);
        if (lane % cpg == 0 && ok[j]) wsum[wave][(j * 64 + lane) / cpg] = s;
    }
    __syncthreads();
    for (int g = threadIdx.x; g < G; g += 256)
        part_out[((long)b * SGN_P + p) * G + g] = ((wsum[0][g] + wsum[1][g]) + wsum[2][g]) + wsum[3][g];
}

// Grid (ceil(max L * C / 8 / 512), B): (mean, rstd) of segment b from its partials, then
// xa = f16(silu((x - mean) * rstd * gamma + beta)) for two 8-channel vectors per thread.
__global__ __launch_bounds__(256) void seg_gn_apply_kernel(const float *x, const int *off, int C, int G, int cpg,
                                                           float eps, const double *part1, const double *part2,
                                                           const float *gamma, const float *beta, _Float16 *xa) {
    __shared__ double red1[64], red2[64];
    __shared__ float2 st[64];
    const int b = blockIdx.y;
    const int s0 = off[b], L = off[b + 1] - s0;
    const long n8 = (long)L * C / 8;
    if ((long)blockIdx.x * 512 >= n8) return;
    const int rows = sgn_rows(L), P = (L + rows - 1) / rows;
    const long n = (long)L * cpg;
    sgn_reduce(part1 + (long)b * SGN_P * G, P, G, red1);
    sgn_reduce(part2 + (long)b * SGN_P * G, P, G, red2);
    if (threadIdx.x < G) {
        const float mean = (float)(red1[threadIdx.x] / (double)n);
        const float variance = (float)(red2[threadIdx.x] / (double)n);
        st[threadIdx.x] = make_float2(mean, 1.0f / sqrtf(variance + eps));
    }
    __syncthreads();
    const float *xs = x + (long)s0 * C;
    _Float16 *xo = xa + (long)s0 * C;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const long e8 = (long)blockIdx.x * 512 + 256 * k + threadIdx.x;
        if (e8 >= n8) break;
        const int c0 = (int)((e8 * 8) % C);
        const float4 u0 = *reinterpret_cast<const float4 *>(xs + e8 * 8);
        const float4 u1 = *reinterpret_cast<const float4 *>(xs + e8 * 8 + 4);
        const float t[8] = {u0.x, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w};
        f16x8 o;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float2 ms = st[(c0 + q) / cpg];
            float y = t[q] - ms.x;
            y = y * ms.y;
            y = y * gamma[c0 + q];
            y = y + beta[c0 + q];
            o[q] = (_Float16)silu_f(y);
        }
        *reinterpret_cast<f16x8 *>(xo + e8 * 8) = o;
    }
}

// ---------------------------------------------------------------- banded attention per segment
// Grid (ceil(max S_b / 16), H, B): 16 queries of ONE segment per workgroup, 16 threads per
// query, so the K / V window in LDS ([i0 - hw, i0 + 15 + hw] clipped to the segment) never
// holds a neighbour's row and the band needs no per-key segment test. RoPE by the position
// inside the segment (one shared [max S_b][32] table). Scores, softmax and P V in the order of
// band_attention_kernel.
constexpr int BA_QB = 16, BA_TQ = 16, BA_HD = 64, BA_MAXHW = 32;
constexpr int BA_KB = BA_QB + 2 * BA_MAXHW;
constexpr int BA_LD = BA_HD + 4;
constexpr int BA_NS = (2 * BA_MAXHW + 1 + BA_TQ - 1) / BA_TQ;

__device__ __forceinline__ float4 rope4(float4 k, float4 cs) {
    return make_float4(k.x * cs.x - k.y * cs.y, k.x * cs.y + k.y * cs.x, k.z * cs.z - k.w * cs.w, k.z * cs.w + k.w * cs.z);
}

__global__ __launch_bounds__(256) void seg_band_attention_kernel(const float *qkv_all, float *out_all, const int *off,
                                                                 int H, int hw, const float2 *rope) {
    __shared__ __attribute__((aligned(16))) float Ks[BA_KB][BA_LD];
    __shared__ __attribute__((aligned(16))) float Vs[BA_KB][BA_HD];
    __shared__ __attribute__((aligned(16))) float Qs[BA_QB][BA_LD];
    __shared__ float Ps[BA_QB][2 * BA_MAXHW + 2];
    const int s0 = off[blockIdx.z], S = off[blockIdx.z + 1] - s0;
    const int h = blockIdx.y, i0 = blockIdx.x * BA_QB, tid = threadIdx.x;
    if (i0 >= S) return;
    const int D = H * BA_HD, ld = 3 * D;
    const float *qkv = qkv_all + (long)s0 * ld;
    float *out = out_all + (long)s0 * D;
    const int kbeg = max(i0 - hw, 0), kend = min(i0 + BA_QB - 1 + hw, S - 1);
    const int nk = kend - kbeg + 1;

    for (int e = tid; e < nk * (BA_HD / 4); e += 256) {
        const int r = e / (BA_HD / 4), c = (e - r * (BA_HD / 4)) * 4;
        const long p = kbeg + r;
        const float4 k = *reinterpret_cast<const float4 *>(qkv + p * ld + D + h * BA_HD + c);
        const float4 cs = *reinterpret_cast<const float4 *>(rope + p * (BA_HD / 2) + c / 2);
        const float4 v = *reinterpret_cast<const float4 *>(qkv + p * ld + 2 * D + h * BA_HD + c);
        *reinterpret_cast<float4 *>(&Ks[r][c]) = rope4(k, cs);
        *reinterpret_cast<float4 *>(&Vs[r][c]) = v;
    }
    for (int e = tid; e < BA_QB * (BA_HD / 4); e += 256) {
        const int r = e / (BA_HD / 4), c = (e - r * (BA_HD / 4)) * 4;
        const long p = min(i0 + r, S - 1);
        const float4 q = *reinterpret_cast<const float4 *>(qkv + p * ld + h * BA_HD + c);
        const float4 cs = *reinterpret_cast<const float4 *>(rope + p * (BA_HD / 2) + c / 2);
        *reinterpret_cast<float4 *>(&Qs[r][c]) = rope4(q, cs);
    }
    __syncthreads();

    const int ql = tid / BA_TQ, t = tid % BA_TQ;
    const int i = i0 + ql;
    const bool active = i < S;
    const int j0 = active ? max(i - hw, 0) : 0;
    const int j1 = active ? min(i + hw, S - 1) : -1;
    float q[BA_HD];
#pragma unroll
    for (int d = 0; d < BA_HD; d += 4) {
        const float4 v = *reinterpret_cast<const float4 *>(&Qs[ql][d]);
        q[d] = v.x, q[d + 1] = v.y, q[d + 2] = v.z, q[d + 3] = v.w;
    }
    float mx = -INFINITY;
    float sc[BA_NS];
#pragma unroll
    for (int n = 0; n < BA_NS; ++n) {
        const int j = j0 + t + BA_TQ * n;
        float s = -INFINITY;
        if (j <= j1) {
            const float *kr = Ks[j - kbeg];
            float a = 0.0f;
#pragma unroll
            for (int d = 0; d < BA_HD; d += 4) {
                const float4 k = *reinterpret_cast<const float4 *>(kr + d);
                a = fmaf(k.x, q[d], a);
                a = fmaf(k.y, q[d + 1], a);
                a = fmaf(k.z, q[d + 2], a);
                a = fmaf(k.w, q[d + 3], a);
            }
            s = a * 0.125f;  // 1/sqrt(64), exact
        }
        sc[n] = s;
        mx = fmaxf(mx, s);
    }
#pragma unroll
    for (int o = 1; o < BA_TQ; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float sum = 0.0f;
#pragma unroll
    for (int n = 0; n < BA_NS; ++n) {
        const int j = j0 + t + BA_TQ * n;
        const float e = (j <= j1) ? expf(sc[n] - mx) : 0.0f;
        sc[n] = e;
        sum += e;
    }
#pragma unroll
    for (int o = 1; o < BA_TQ; o <<= 1) sum += __shfl_xor(sum, o);
    const float inv = 1.0f / sum;
#pragma unroll
    for (int n = 0; n < BA_NS; ++n) {
        const int j = j0 + t + BA_TQ * n;
        if (j <= j1) Ps[ql][j - j0] = sc[n] * inv;
    }
    __syncthreads();
    if (!active) return;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = j0; j <= j1; ++j) {
        const float p = Ps[ql][j - j0];
        const float4 v = *reinterpret_cast<const float4 *>(&Vs[j - kbeg][4 * t]);
        o.x = fmaf(p, v.x, o.x);
        o.y = fmaf(p, v.y, o.y);
        o.z = fmaf(p, v.z, o.z);
        o.w = fmaf(p, v.w, o.w);
    }
    *reinterpret_cast<float4 *>(out + (long)i * D + h * BA_HD + 4 * t) = o;
}

// ---------------------------------------------------------------- conditioning, B voices
// y[b][r] = W[r][:] . silu(e[b]) + bias[r]: one wave per row r, each W element loaded once and
// used for all B voices (B accumulators in registers); per voice the k order and the lane
// tree of cond_gemv_kernel.
__global__ __launch_bounds__(256) void cond_gemv_batch_kernel(const float *W, const float *bias, const float *e,
                                                              int R, int A, int B, float *y, int e_f16) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    float a[kSegMax];
#pragma unroll
    for (int b = 0; b < kSegMax; ++b) a[b] = 0.0f;
    for (int k = lane; k < A; k += 64) {
        const float w = W[(long)r * A + k];
#pragma unroll
        for (int b = 0; b < kSegMax; ++b) {
            if (b < B) {
                float se = silu_f(e[(long)b * A + k]);
                if (e_f16) se = (float)(_Float16)se;
                a[b] = fmaf(w, se, a[b]);
            }
        }
    }
    const float br = bias[r];
#pragma unroll
    for (int b = 0; b < kSegMax; ++b) {
        float s = a[b];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0 && b < B) y[(long)b * R + r] = s + br;
    }
}

}  // namespace

void launch_seg_gemm(const SegGemmArgs &a, int epi, hipStream_t s) {
    const dim3 grid((a.N + SG_T - 1) / SG_T, (a.M - a.m_begin + SG_T - 1) / SG_T);
    auto go = [&](auto kg) {
        constexpr int KG = decltype(kg)::value;
        if (epi == EPI_GATED)
            hipLaunchKernelGGL((seg_gemm_kernel<EPI_GATED, KG>), grid, dim3(256), 0, s, a);
        else
            hipLaunchKernelGGL((seg_gemm_kernel<EPI_CONVT_SNAKE, KG>), grid, dim3(256), 0, s, a);
    };
    switch (a.kg) {
        case 1: go(std::integral_constant<int, 1>{}); break;
        case 2: go(std::integral_constant<int, 2>{}); break;
        default: go(std::integral_constant<int, 4>{}); break;
    }
}

void launch_seg_conv_f16(const ConvArgs &a, const int *off, int B, hipStream_t s) {
    const dim3 grid((a.Cout + CV_BN - 1) / CV_BN, (a.L + CV_BM - 1) / CV_BM);
    hipLaunchKernelGGL(seg_conv_f16_kernel, grid, dim3(256), 0, s, a, off, B);
}

void launch_seg_rownorm(const float *x, float *y, int M, int D, float eps, const float *shift, const float *scale,
                        int ld, const int *off, int B, hipStream_t s) {
    const dim3 grid((M + 3) / 4);
    switch (D / 64) {
#define RN(P)                                                                                                  \
    case P:                                                                                                    \
        hipLaunchKernelGGL(seg_rownorm_kernel<P>, grid, dim3(256), 0, s, x, y, M, eps, shift, scale, ld, off, B); \
        break;
        RN(1) RN(2) RN(3) RN(4) RN(5) RN(6) RN(7) RN(8) RN(9) RN(10) RN(11) RN(12) RN(13) RN(14) RN(15) RN(16)
#undef RN
        default: break;  // refused at load (codec.cpp: D % 64 == 0, D <= 1024)
    }
}

void launch_seg_groupnorm_apply(const float *x, const int *off, int B, int Lmax, int C, int G, float eps,
                                const float *gamma, const float *beta, double *part, _Float16 *xa, hipStream_t s) {
    const int cpg = C / G;
    // slices of the longest cut: a segment has at most min(128, ceil(L / 4)) of them
    const dim3 gp(std::min(SGN_P, (Lmax + 3) / 4), B);
    double *part1 = part, *part2 = part + (long)kSegMax * SGN_P * 64;
    switch ((C + 63) / 64) {
#define GP(J)                                                                                                       \
    case J:                                                                                                         \
        hipLaunchKernelGGL((seg_gn_partial_kernel<1, J>), gp, dim3(256), 0, s, x, off, C, G, cpg,                   \
                           (const double *)part1, part1);                                                           \
        hipLaunchKernelGGL((seg_gn_partial_kernel<2, J>), gp, dim3(256), 0, s, x, off, C, G, cpg,                   \
                           (const double *)part1, part2);                                                           \
        break;
        GP(1) GP(2) GP(3) GP(4) GP(5) GP(6) GP(7) GP(8) GP(9) GP(10) GP(11) GP(12) GP(13) GP(14) GP(15) GP(16)
#undef GP
        default: return;  // C <= 1024 (codec.cpp refuses larger)
    }
    const long n8 = (long)Lmax * C / 8;
    hipLaunchKernelGGL(seg_gn_apply_kernel, dim3((unsigned)((n8 + 511) / 512), B), dim3(256), 0, s, x, off, C, G, cpg,
                       eps, (const double *)part1, (const double *)part2, gamma, beta, xa);
}

void launch_seg_band_attention(const float *qkv, float *out, const int *off, int B, int Smax, int H, int window,
                               const float2 *rope, hipStream_t s) {
    const dim3 grid((Smax + BA_QB - 1) / BA_QB, H, B);
    hipLaunchKernelGGL(seg_band_attention_kernel, grid, dim3(256), 0, s, qkv, out, off, H, window / 2, rope);
}

void launch_cond_gemv_batch(const float *W, const float *b, const float *e, int R, int A, int B, float *y, int e_f16,
                            hipStream_t s) {
    hipLaunchKernelGGL(cond_gemv_batch_kernel, dim3((R + 3) / 4), dim3(256), 0, s, W, b, e, R, A, B, y, e_f16);
}

}  // namespace mio
