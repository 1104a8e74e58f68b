// The LLM weight types, stated once: the ggml type ids under their names, the predicates the
// kernels branch on, the split layout (the layout the gfx950 kernels stream, written by
// quant.cpp's to_split) as a table, and the q|k / attn_v type pairs the fused launches exist for.
// No dependencies; host and device code include it (llm_kernels.h, quant.h, gguf.h).
//
// Split layout of one [R][K] matrix: up to four planes, each row-major with its own row stride.
// Bytes of one block (256 weights of a K-quant, 32 of Q8_0, 1 of BF16) in each plane:
//
//   Q8_0 : qs 32 int8        | d  2 f16
//   Q3_K : q  64 u8          | h  32 u8 high-bit plane | sc 16 i8 (piece order)     | d 2 f16
//   Q4_K : qs 128 u8 nibbles | hd 16 = {d, dmin, 4 x 24-bit scale pairs}
//   Q5_K : qs 128 u8 nibbles | qh 32 u8 fifth-bit plane | hd 16 as Q4_K's
//   Q6_K : ql 128 u8         | qh 64 u8                | sc 16 i8 (lane-pair order) | d 2 f16
//   BF16 : 2
//
// Same bytes per weight as GGUF, except Q3_K: 114 B per superblock for the GGUF's 110 (quant.h).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MIO_WT_FN __host__ __device__ constexpr
#else
#define MIO_WT_FN constexpr
#endif

namespace mio {

// ggml tensor type ids (public ggml enum values).
enum GgmlType : unsigned {
    GGML_F32 = 0,
    GGML_F16 = 1,
    GGML_Q4_0 = 2,
    GGML_Q5_0 = 6,
    GGML_Q8_0 = 8,
    GGML_Q3_K = 11,
    GGML_Q4_K = 12,
    GGML_Q5_K = 13,
    GGML_Q6_K = 14,
    GGML_Q8_K = 15,
    GGML_I8 = 24,
    GGML_I16 = 25,
    GGML_I32 = 26,
    GGML_BF16 = 30,
};

// The types a weight matrix may have on the device (Q4_0 / Q5_0 files are repacked to Q8_0).
constexpr int kWeightTypes[] = {GGML_Q8_0, GGML_Q3_K, GGML_Q4_K, GGML_Q5_K, GGML_Q6_K, GGML_BF16};
constexpr int kNumWeightTypes = sizeof(kWeightTypes) / sizeof(kWeightTypes[0]);

// 256-weight superblocks
MIO_WT_FN bool is_kquant(int t) { return t == GGML_Q3_K || t == GGML_Q4_K || t == GGML_Q5_K || t == GGML_Q6_K; }
// superblock header {d, dmin, scales | mins}: the mins go against the activation's bsums
MIO_WT_FN bool has_mins(int t) { return t == GGML_Q4_K || t == GGML_Q5_K; }
// superblock of int8 scales and one d: no mins
MIO_WT_FN bool scale_only(int t) { return t == GGML_Q6_K || t == GGML_Q3_K; }
// one block (Q8_0) or one piece (BF16) per lane: float terms, summed over 8 lanes by sum8_f
MIO_WT_FN bool lane_blocks(int t) { return t == GGML_Q8_0 || t == GGML_BF16; }
// activations are streamed as bf16 records (2 bytes per element)
MIO_WT_FN bool bf16_records(int t) { return t == GGML_BF16; }

// ------------------------------------------------------------------ split layout
constexpr int kMaxPlanes = 4;

// weights per block: K is a multiple of it (0: not a weight type)
MIO_WT_FN int block_elems(int t) { return is_kquant(t) ? 256 : t == GGML_Q8_0 ? 32 : t == GGML_BF16 ? 1 : 0; }
MIO_WT_FN bool is_weight_type(int t) { return block_elems(t) != 0; }

// bytes of one block in plane p (0: the type has no such plane)
MIO_WT_FN int plane_block_bytes(int t, int p) {
    if (p < 0 || p >= kMaxPlanes) return 0;
    switch (t) {
        case GGML_Q8_0: { const int b[kMaxPlanes] = {32, 2, 0, 0}; return b[p]; }
        case GGML_Q3_K: { const int b[kMaxPlanes] = {64, 32, 16, 2}; return b[p]; }
        case GGML_Q4_K: { const int b[kMaxPlanes] = {128, 16, 0, 0}; return b[p]; }
        case GGML_Q5_K: { const int b[kMaxPlanes] = {128, 32, 16, 0}; return b[p]; }
        case GGML_Q6_K: { const int b[kMaxPlanes] = {128, 64, 16, 2}; return b[p]; }
        case GGML_BF16: { const int b[kMaxPlanes] = {2, 0, 0, 0}; return b[p]; }
        default: return 0;
    }
}
MIO_WT_FN int num_planes(int t) {
    int n = 0;
    while (n < kMaxPlanes && plane_block_bytes(t, n)) ++n;
    return n;
}
// row stride of plane p of a matrix with rows of k weights
MIO_WT_FN unsigned long long plane_row_bytes(int t, long long k, int p) {
    return is_weight_type(t) ? (unsigned long long)(k / block_elems(t)) * plane_block_bytes(t, p) : 0;
}
// all planes of one block / one row
MIO_WT_FN int block_bytes(int t) {
    int n = 0;
    for (int p = 0; p < kMaxPlanes; ++p) n += plane_block_bytes(t, p);
    return n;
}
MIO_WT_FN unsigned long long row_bytes(int t, long long k) {
    return is_weight_type(t) ? (unsigned long long)(k / block_elems(t)) * block_bytes(t) : 0;
}
// Pin of a stride written out in a kernel: plane p's row stride is k / div * mul, checked at one
// superblock and at a K of nine (static_assert(stride_is(GGML_Q6_K, 1, 1, 4)) beside `W.k / 4`).
MIO_WT_FN bool stride_is(int t, int p, int mul, int div) {
    return plane_row_bytes(t, 256, p) == 256ull / div * mul && plane_row_bytes(t, 2304, p) == 2304ull / div * mul;
}

static_assert(block_bytes(GGML_Q3_K) == 114 && block_elems(GGML_Q3_K) == 256 && num_planes(GGML_Q3_K) == 4, "Q3_K");
static_assert(block_bytes(GGML_Q4_K) == 144 && block_elems(GGML_Q4_K) == 256 && num_planes(GGML_Q4_K) == 2, "Q4_K");
static_assert(block_bytes(GGML_Q5_K) == 176 && block_elems(GGML_Q5_K) == 256 && num_planes(GGML_Q5_K) == 3, "Q5_K");
static_assert(block_bytes(GGML_Q6_K) == 210 && block_elems(GGML_Q6_K) == 256 && num_planes(GGML_Q6_K) == 4, "Q6_K");
static_assert(block_bytes(GGML_Q8_0) == 34 && block_elems(GGML_Q8_0) == 32 && num_planes(GGML_Q8_0) == 2, "Q8_0");
static_assert(block_bytes(GGML_BF16) == 2 && block_elems(GGML_BF16) == 1 && num_planes(GGML_BF16) == 1, "BF16");
static_assert(row_bytes(GGML_Q6_K, 2304) == 9 * 210 && plane_row_bytes(GGML_Q6_K, 2304, 1) == 2304 / 4, "rows");
static_assert(!is_weight_type(GGML_F16) && !is_weight_type(GGML_Q4_0) && num_planes(GGML_F32) == 0, "others");

// ------------------------------------------------------------------ q|k beside attn_v
// The (q|k type, attn_v type) pairs the q|k|v launches are instantiated for: v of q|k's own type,
// Q6_K beside Q4_K / Q5_K (the *_K_M mixes' use_more_bits layers), Q4_K beside Q6_K, Q4_K / Q5_K
// beside Q3_K (Q3_K_M / Q3_K_L). In the order the launches first use them, which fixes each
// kernel's place in its code object: append, do not sort.
struct QkvTypes {
    int qk, v;
};
constexpr QkvTypes kQkvTypes[] = {
    {GGML_Q4_K, GGML_Q4_K}, {GGML_Q4_K, GGML_Q6_K}, {GGML_Q5_K, GGML_Q5_K}, {GGML_Q5_K, GGML_Q6_K},
    {GGML_Q6_K, GGML_Q6_K}, {GGML_Q6_K, GGML_Q4_K}, {GGML_Q8_0, GGML_Q8_0}, {GGML_Q3_K, GGML_Q3_K},
    {GGML_Q3_K, GGML_Q4_K}, {GGML_Q3_K, GGML_Q5_K}, {GGML_BF16, GGML_BF16},
};
constexpr int kNumQkvTypes = sizeof(kQkvTypes) / sizeof(kQkvTypes[0]);
constexpr bool attn_v_supported(int tq, int tv) {
    for (int i = 0; i < kNumQkvTypes; ++i)
        if (kQkvTypes[i].qk == tq && kQkvTypes[i].v == tv) return true;
    return false;
}

}  // namespace mio
