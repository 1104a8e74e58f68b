// Device helpers of the Q8_0 K/V cache (KvQ8, llm_kernels.h), the counterparts of kv_issue /
// kv_stage / kv_stage_row (llm_device.h) for the launches of llm_attention_q8.hip.
//
// A cache row of one kv head is HD int8 codes and HD / 32 f16 scales, in two planes. The row
// quantizer is ggml's quantize_row_q8_0_ref on the f16-exact k / v values the F16 cache would
// store: per 32 values d = amax / 127 (f32), id = d ? 1 / d : 0, q = roundf(x * id) (half away
// from zero), d stored as f16 (round to nearest even). Attention consumes f16(float(d_f16) * q),
// round to nearest even (the product is exact in f32: 11 x 8 significant bits), written into the
// same swizzled f16 images attend_chunk_mfma reads: the MFMA body, the chunk records and the merge
// are the F16 cache's, and the two cache types differ in this one rounding of the cached rows.
#pragma once
#include "llm_device.h"

namespace mio {
namespace {

// Work split of a chunk's rows: a thread takes 16-code units (16 B of codes, inside one 32-block,
// so one scale each), half as many 16-byte loads per thread as AttM<HD>::VI, and expands each
// into two 8-value f16 chunks of the images.
template <int HD>
struct KvQ8M {
    using A = AttM<HD>;
    static constexpr int UR = HD / 16;              // units per row
    static constexpr int UN = ATT_CHUNK * UR;       // units per chunk image
    static constexpr int VQ = (UN + A::NT - 1) / A::NT;  // units of K (and of V) each thread stages
    static constexpr int SB = HD / 32 * 2;          // scale bytes per row (4 or 8: whole 32-bit words)
    static_assert(HD % 64 == 0, "two scales per 32-bit word");
};

template <int HD>
struct KvQ8Regs {
    u32x4 kq[KvQ8M<HD>::VQ], vq[KvQ8M<HD>::VQ];   // 16 codes
    uint32_t ks[KvQ8M<HD>::VQ], vs[KvQ8M<HD>::VQ];  // the 32-bit word holding the unit's f16 scale
};

// This thread's units of the chunk's rows t0 .. t0 + ATT_CHUNK - 1 of one kv head, issued early.
// As kv_issue reasons it: rows past pos are masked positions whose probability is 0, but 0 x NaN
// and 0 x Inf are NaN in the P.V MFMA, so whatever the planes hold there must stage as finite
// values. All four loads are range-checked buffer loads over the written rows alone ([0, pos), or
// [0, pos] where an earlier launch wrote row pos: the prefill): a row past them reads codes 0 and
// scale 0, which dequantize to +0. A scale's word never straddles the last written row (SB is a
// multiple of 4).
template <int HD>
__device__ __forceinline__ void kv_issue_q8(const int8_t *kq, const _Float16 *ks, const int8_t *vq, const _Float16 *vs,
                                            int t0, int pos, KvQ8Regs<HD> &r, bool row_pos_written = false) {
    using Q = KvQ8M<HD>;
    const uint32_t rows = (uint32_t)(pos + (row_pos_written ? 1 : 0));
    const __amdgpu_buffer_rsrc_t kqr = rsrc(kq, rows * (uint32_t)HD), vqr = rsrc(vq, rows * (uint32_t)HD);
    const __amdgpu_buffer_rsrc_t ksr = rsrc(ks, rows * (uint32_t)Q::SB), vsr = rsrc(vs, rows * (uint32_t)Q::SB);
#pragma unroll
    for (int it = 0; it < Q::VQ; ++it) {
        const int u = it * Q::A::NT + (int)MIO_TIDX, row = u / Q::UR, c = u % Q::UR;
        // a thread past the chunk's units (32-position chunks at hd 64): out of every range
        const bool live = Q::UN % Q::A::NT == 0 || u < Q::UN;
        const uint32_t oq = live ? (uint32_t)(t0 + row) * (uint32_t)HD + 16u * c : 0x80000000u;
        const uint32_t os = live ? (uint32_t)(t0 + row) * (uint32_t)Q::SB + 4u * (c >> 2) : 0x80000000u;
        r.kq[it] = __builtin_amdgcn_raw_buffer_load_b128(kqr, oq, 0, 0);
        r.ks[it] = __builtin_amdgcn_raw_buffer_load_b32(ksr, os, 0, 0);
        r.vq[it] = __builtin_amdgcn_raw_buffer_load_b128(vqr, oq, 0, 0);
        r.vs[it] = __builtin_amdgcn_raw_buffer_load_b32(vsr, os, 0, 0);
    }
}

// 16 codes x their scale -> two 8-value f16 chunks: int8 -> f32 (exact), x d (exact), f16 RNE
__device__ __forceinline__ void q8_dequant16(const u32x4 &q, uint32_t sword, bool hi, h8 &a, h8 &b) {
    const float d = (float)__builtin_bit_cast(_Float16, (uint16_t)(hi ? sword >> 16 : sword & 0xFFFFu));
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        a[e] = (_Float16)(d * (float)(int)(int8_t)(q[e >> 2] >> (8 * (e & 3))));
        b[e] = (_Float16)(d * (float)(int)(int8_t)(q[2 + (e >> 2)] >> (8 * (e & 3))));
    }
}

// The units into the images, dequantized in registers; row `skip` (the position being decoded) is
// staged by the wave that quantized it (kv_stage_row on its dequantized values).
// A unit is logical chunks 2 c and 2 c + 1 of its row. The 8-lane groups of one ds_write_b128 must
// sit on 8 distinct 16-byte bank slots (AttM: slot = chunk ^ f(row), mod 8): at hd 128 a group is
// units 0..7 of one row, whose even chunks alone collide mod 8, so units 4..7 store their odd
// chunk first (0 2 4 6 9 11 13 15); at hd 64 a group is two rows of 4 units sharing f, and the odd
// row stores its odd chunks first (0 2 4 6 | 1 3 5 7).
template <int HD>
__device__ __forceinline__ void kv_stage_q8(const KvQ8Regs<HD> &r, int skip, char *kimg, char *vimg) {
    using Q = KvQ8M<HD>;
    using A = AttM<HD>;
#pragma unroll
    for (int it = 0; it < Q::VQ; ++it) {
        const int u = it * A::NT + (int)MIO_TIDX, row = u / Q::UR, c = u % Q::UR;
        if ((Q::UN % A::NT == 0 || u < Q::UN) && row != skip) {
            const bool hi = (c >> 1) & 1;
            const bool odd_first = HD == 128 ? ((c >> 2) & 1) != 0 : (row & 1) != 0;
            const int c0 = 2 * c + (odd_first ? 1 : 0), c1 = 2 * c + (odd_first ? 0 : 1);
            h8 a, b;
            q8_dequant16(r.kq[it], r.ks[it], hi, a, b);
            *reinterpret_cast<h8 *>(kimg + row * A::RB + 16 * (c0 ^ A::fk(row))) = odd_first ? b : a;
            *reinterpret_cast<h8 *>(kimg + row * A::RB + 16 * (c1 ^ A::fk(row))) = odd_first ? a : b;
            q8_dequant16(r.vq[it], r.vs[it], hi, a, b);
            *reinterpret_cast<h8 *>(vimg + row * A::RB + 16 * (c0 ^ A::fv(row))) = odd_first ? b : a;
            *reinterpret_cast<h8 *>(vimg + row * A::RB + 16 * (c1 ^ A::fv(row))) = odd_first ? a : b;
        }
    }
}

// One wave quantizes a new cache row of one kv head: lane holds the f16-exact values x[i] = row
// element lane + 64 i, so each 32-lane half of a register is one Q8_0 block and its amax is five
// lane exchanges inside the half. Codes and scales go to the planes with vector stores (q, s: the
// row's codes and scales); x is left holding the dequantized values the images take, so the step
// that appends the row sees it exactly as every later step and the prefill will.
template <int HD>
__device__ __forceinline__ void q8_quant_row(float (&x)[HD / 64], int8_t *q, _Float16 *s) {
    const int lane = MIO_TIDX & 63;
#pragma unroll
    for (int i = 0; i < HD / 64; ++i) {
        float am = fabsf(x[i]);
        am = fmaxf(am, xor_lane<16>(am));
        am = fmaxf(am, xor_lane<8>(am));
        am = fmaxf(am, xor_lane<4>(am));
        am = fmaxf(am, xor_lane<2>(am));
        am = fmaxf(am, xor_lane<1>(am));
        const float d = am / 127.0f;
        const float id = d != 0.0f ? 1.0f / d : 0.0f;
        const int qi = (int)roundf(x[i] * id);
        const _Float16 dh = (_Float16)d;
        q[lane + 64 * i] = (int8_t)qi;
        if ((lane & 31) == 0) s[(lane >> 5) + 2 * i] = dh;
        x[i] = f16r((float)dh * (float)qi);  // of the stored code: a code 0 is +0 whatever x's sign
    }
}

}  // namespace
}  // namespace mio
