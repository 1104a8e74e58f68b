// ggml block quant formats (public ggml spec) on the host:
// fp16 conversion, row quantizers (used to make synthetic Q8_0 / Q4_K_M / Q5_K_M models),
// row dequantizers (embedding get_rows), and the re-layout of a GGUF quantized matrix
// into the "split" layout the gfx950 matvec kernels stream. The layout's planes and their row
// strides are the table of csrc/weight_types.h (plane_row_bytes); the order of the bytes inside
// a plane is to_split's, restated by the dequantizers of the kernels (llm_device.h dequant_elem).
//
// Same bytes per weight as GGUF (algorithmic bytes unchanged; Q3_K: 114 B per superblock for
// the GGUF's 110, below); each row's quant payload becomes one contiguous, 16-B aligned run, so
// one wave reads a row with 16 B per lane (Q3_K: 8 B).
//
// Q3_K regroups the bits inside a superblock (the same 256 codes and 16 scales, permuted), so a
// matvec lane's 32 weights are two whole sub-blocks, 32 elements apart, as Q4_K's and Q5_K's are.
// Piece pc (0..7) holds the runs lo = elements 64 (pc >> 1) + 16 (pc & 1) .. + 15 (sub-block
// 4 (pc >> 1) + (pc & 1)) and hi = lo + 32 (sub-block + 2). The pieces are stored at position
// P(pc) = 4 (pc & 1) + (pc >> 1) of each plane - the even pieces, then the odd ones - so the
// matrix-core tiles, whose lanes hold the pieces of one parity, read them with 16-B loads:
//   q  : 64 B, piece at byte 8 P: dword 0 = run lo, dword 1 = run hi; the 2-bit code of the
//        run's element i sits in byte i % 4 at bits 2 (i / 4), so (dword >> 2 k) & 0x03030303 are
//        the codes of elements 4 k .. 4 k + 3, one per byte, as the dot4 instructions take them
//   h  : 32 B, piece at byte 4 P: one dword; hmask's bit of run lo's element i sits in byte i % 4
//        at bit i / 4, run hi's at bit 4 + i / 4 (1 = the code counts + 4, as in hmask)
//   sc : 16 B, piece at byte 2 P: the two sub-blocks' 6-bit scales unpacked and the 32 taken off,
//        int8 in [-32, 31] (run lo, run hi)
//   d  : the superblock's f16 d
// 114 B, not the 112 B of the packed 12 scale bytes + d rounded up to a header: with int8
// scales no lane runs ggml's kmask shuffle per unit, as Q6_K's lanes do not; 3.6 % more bytes
// than the GGUF, which mio_hip_llm_weight_bytes counts.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "weight_types.h"

namespace mio {

#pragma pack(push, 1)
struct BlockQ8_0 {
    uint16_t d;
    int8_t qs[32];
};
// llama-quantize's fallbacks for rows whose length is not a multiple of 256 (Q4_K -> Q5_0,
// llama.cpp llama-quant.cpp) and plain Q4_0 files: 32 weights per block, codes q - 8 / q - 16.
struct BlockQ4_0 {
    uint16_t d;
    uint8_t qs[16];
};
struct BlockQ5_0 {
    uint16_t d;
    uint8_t qh[4];
    uint8_t qs[16];
};
// 16 sub-blocks of 16 weights: weight e has the 2-bit code (qs[32 (e / 128) + e % 32] >> 2 ((e / 32)
// % 4)) & 3 and the high bit (hmask[e % 32] >> (e / 32)) & 1, q = code + 4 high - 4; sub-block j's
// 6-bit scale is ((scales[j % 8] >> 4 (j / 8)) & 0xF) | (((scales[8 + j % 4] >> 2 (j / 4)) & 3) << 4),
// used as scale - 32
struct BlockQ3_K {
    uint8_t hmask[32];
    uint8_t qs[64];
    uint8_t scales[12];
    uint16_t d;
};
struct BlockQ4_K {
    uint16_t d, dmin;
    uint8_t scales[12];
    uint8_t qs[128];
};
// Q4_K plus one plane of fifth bits: weight e of sub-block j = e / 32 has bit (qh[e % 32] >> j) & 1
struct BlockQ5_K {
    uint16_t d, dmin;
    uint8_t scales[12];
    uint8_t qh[32];
    uint8_t qs[128];
};
struct BlockQ6_K {
    uint8_t ql[128];
    uint8_t qh[64];
    int8_t scales[16];
    uint16_t d;
};
#pragma pack(pop)
static_assert(sizeof(BlockQ8_0) == 34, "q8_0");
static_assert(sizeof(BlockQ4_0) == 18, "q4_0");
static_assert(sizeof(BlockQ5_0) == 22, "q5_0");
static_assert(sizeof(BlockQ3_K) == 110, "q3_K");
static_assert(sizeof(BlockQ4_K) == 144, "q4_K");
static_assert(sizeof(BlockQ5_K) == 176, "q5_K");
static_assert(sizeof(BlockQ6_K) == 210, "q6_K");

float fp16_to_f32(uint16_t h);
uint16_t f32_to_fp16(float f);  // round to nearest even
uint16_t f32_to_bf16(float f);  // ggml_compute_fp32_to_bf16

void quantize_row_q8_0(const float *x, void *y, int64_t k);
void quantize_row_q4_0(const float *x, void *y, int64_t k);
void quantize_row_q5_0(const float *x, void *y, int64_t k);
void quantize_row_q3_K(const float *x, void *y, int64_t k);
void quantize_row_q4_K(const float *x, void *y, int64_t k);
void quantize_row_q5_K(const float *x, void *y, int64_t k);
void quantize_row_q6_K(const float *x, void *y, int64_t k);
bool quantize_row(uint32_t type, const float *x, void *y, int64_t k);
bool dequantize_row(uint32_t type, const void *x, float *y, int64_t k);

// Q4_0 / Q5_0 rows as Q8_0 rows, losslessly: a block's codes x - 8 (Q4_0) or x - 16 (Q5_0)
// lie in [-16, 15] and keep their f16 scale, and ggml's vec_dot_q4_0_q8_0 / vec_dot_q5_0_q8_0
// (vec_dot_type Q8_0, sumi * (d_w * d_a) per block) equal vec_dot_q8_0_q8_0 on the repacked
// block term for term, as dequantize_row does. dst: R * (K / 32) * 34 bytes.
bool repack_to_q8_0(uint32_t type, const void *src, int64_t rows, int64_t k, void *dst);
bool repacks_to_q8_0(uint32_t type);

// Split layout of one [R][K] matrix (offsets in bytes from the tensor's base).
struct SplitLayout {
    uint32_t type = 0;
    int64_t rows = 0, k = 0;
    size_t off[4] = {0, 0, 0, 0};
    size_t bytes = 0;
};
SplitLayout split_layout(uint32_t type, int64_t rows, int64_t k);
// GGUF rows -> split layout (dst has layout.bytes). Returns false on unsupported type.
bool to_split(uint32_t type, const void *src, int64_t rows, int64_t k, uint8_t *dst);

}  // namespace mio
