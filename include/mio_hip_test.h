/* Test-support C-ABI: libmiotts_test.so (csrc/testlib/), built beside libmiotts.so and linked
 * to it; the product library exports none of these. Used by tests/, bench.py and tools/:
 * synthetic model files (no real GGUF exists offline) and parity entry points of the kernels. */
#ifndef MIO_HIP_TEST_H
#define MIO_HIP_TEST_H

#include "mio_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What guarded outputs of the parity entry points are filled with before a launch: quiet NaNs
 * with a payload, so an element no thread wrote is recognisable. */
#define MIO_DEBUG_SENTINEL_F32 0x7FC5A5A5u
#define MIO_DEBUG_SENTINEL_F16 0x7E5Au

/* Parity helpers: y[rows] = W x for a GGUF-layout quantized matrix (gguf_rows, ggml type
 * 8/12/13/14) with x re-quantized to the ggml vec_dot_type, on the GPU matvec kernels; and
 * the host quantizer used to build synthetic models (ggml block layout out).
 * mio_hip_debug_matvec, _swiglu, _group and _mmq keep their device output between two 256-byte
 * guard zones and fill guards and output with MIO_DEBUG_SENTINEL_F32 before the launch (mmq mode
 * 1, whose y is in/out: the caller's values between the guards): a row no wave wrote comes back
 * as the sentinel, and a guard zone that changed is MIO_ERR_HIP with a message naming the zone
 * ("before row 0" / "after the last row"). tests/test_rowdot_edges_gpu.py runs them on blocks
 * built from their fields at the integer ceilings (tests/np_rowdot.py: every code, scale and min
 * at its maximum, d / dmin negative, -0, f16-subnormal and 65504, scales and codes of -128,
 * single sub-blocks, random bytes) against an exact integer reference with a counted bound. */
int mio_hip_debug_matvec(mio_hip_device *d, uint32_t type, const void *gguf_rows, int rows, int k,
                         const float *x, float *y);
/* The same with the gate|up launch's row pairs and epilogue: y = silu(Wgate x) * (Wup x). */
int mio_hip_debug_matvec_swiglu(mio_hip_device *d, uint32_t type, const void *gguf_gate, const void *gguf_up, int rows,
                                int k, const float *x, float *y);
/* Either of the two on the decode step's single-group row stream: every wave's share is one
 * register group of su units (a unit = one pass of one row of one matrix; su 2, 3, 4, 6 for
 * k <= 2048, su even with gguf_up; su 3 for 2048 < k <= 6144 without gguf_up), rows split over
 * `grid` workgroups of 8 waves the way the launches split them. gguf_up NULL: y = W x, else
 * the SwiGLU form. MIO_ERR_INVALID where a wave would own more than su units or no such
 * instantiation exists. The outputs equal mio_hip_debug_matvec / _swiglu's bit for bit. */
int mio_hip_debug_matvec_group(mio_hip_device *d, uint32_t type, const void *gguf_gate, const void *gguf_up, int rows,
                               int k, int su, int grid, const float *x, float *y);
int mio_quantize_rows(uint32_t type, const float *x, int rows, int k, void *out);
/* The host dequantizer (ggml dequantize_row_* expression order) on rows of ggml blocks:
 * out[rows][k] f32. */
int mio_dequantize_rows(uint32_t type, const void *rows_bytes, int rows, int k, float *out);
/* The split layout the kernels stream (csrc/host/quant.h) of rows of ggml blocks, on the host:
 * *nbytes = its size, off[4] = the planes' byte offsets; out NULL returns those alone. */
int mio_debug_to_split(uint32_t type, const void *rows_bytes, int rows, int k, uint8_t *out, uint64_t *nbytes,
                       uint64_t *off);
/* The weight-type table (csrc/weight_types.h) as the host reads it, no GPU: for a [rows][k] matrix
 * of a device weight type (8, 11..14, 30), stride[4] = the split layout's plane row strides in
 * bytes (0: no such plane), off[4] = the planes' offsets, moved[4] = the bytes by which taking
 * rows [r0, r0 + n) (qmat_rows) moves each plane pointer. */
int mio_debug_weight_layout(uint32_t type, int rows, int k, int r0, int n, uint64_t *stride, uint64_t *off,
                            uint64_t *moved);
/* 1 where the q|k|v launches exist for attn_v of ggml type tv beside q|k of type tq, else 0. */
int mio_debug_attn_v_supported(int tq, int tv);
/* The decode step's activation quantizer (one 512-thread workgroup, the kernels' own prologue
 * code) on x[k]: type 12 -> Q8_K, 8 -> Q8_0, 30 -> bf16 rounding; w != NULL: RMSNorm(x, eps) * w
 * first; sc1 != 0: the activation loaded the way an in-launch hand-off loads it. Out, the
 * workgroup's LDS record: qs[2k] bytes (int8 codes in the first k, or k bf16 values), d[k/32 + 8]
 * (one per superblock / block), bs[k/16 + 8] (Q8_K bsums); entries the kind does not write are
 * undefined. */
int mio_hip_debug_act_quant(mio_hip_device *d, uint32_t type, const float *x, const float *w, int k, float eps,
                            int sc1, int8_t *qs, float *dd, int16_t *bs);
/* Parity helper: y[t][rows] = W x[t] for nt activation rows x[t][k] on the batched-prefill
 * matmul (int8 MFMA, csrc/hip/llm_mmq.hip); each row equals mio_hip_debug_matvec of x[t].
 * mode 0: y = W x; 1: y = W x + y (y in/out, the residual epilogue); 2: y = silu(W x) *
 * (Wup x) with gguf_up the up matrix (the SwiGLU epilogue). */
int mio_hip_debug_mmq(mio_hip_device *d, uint32_t type, const void *gguf_rows, int rows, int k,
                      const float *x, int nt, int mode, const void *gguf_up, float *y);

/* ---------------- LLM attention on injected K/V ----------------
 * The inverse of mio_hip_llm_kv_rows: f16 bit patterns k, v [n_kv][n_pos][head_dim] are written to
 * cache positions [p0, p0 + n_pos) of layer il. */
int mio_hip_llm_set_kv_rows(mio_hip_llm *m, int il, int p0, int n_pos, const uint16_t *k, const uint16_t *v);
/* One attention launch of layer il at position pos on the raw q|k|v row qkv[(H + 2 Hkv) * hd]
 * (the projections' output: bias, q/k norm, RoPE and the f16 rounding are the launch's own):
 * which = 1 the attention launch, 10 the attention + O launch (MIO_ERR_UNSUPPORTED where the
 * head shape has none; any other value too). att[H * hd] receives the merged attention output.
 * Cache row pos of the layer is written, the decode state is left at pos (eval / generate set
 * their own). A short-conv layer is refused with MIO_ERR_INVALID. */
int mio_hip_llm_debug_attention(mio_hip_llm *m, int il, int pos, int which, const float *qkv, float *att);

/* The polled words of the fused attention launches' hand-offs: words[3 * n_kv] receives, per kv
 * head, the q row counter, the q|k|v row counter and the chunk arrival word. Every one is 0 between
 * decode steps. reset != 0: the runner's counter reset runs first. */
int mio_hip_llm_handoff_words(mio_hip_llm *m, int reset, int32_t *words);

/* ---------------- the sampler chain on an injected logits row ----------------
 * One launch of the chain kernel (penalties -> top-k -> top-p -> min-p -> draw, mio_hip.h
 * mio_sampling) followed by the flush sampler that takes its token: logits[n_vocab] is the row,
 * history[n_history] the tokens the run is taken to have sampled before `step` (oldest first;
 * the launch reads the last repeat_last_n of them; step >= n_history, step < n_ctx), the
 * window is [lo, hi) exactly (0 <= lo < n_vocab, hi <= n_vocab; hi <= lo: empty, the token is
 * lo). *token is the sampled id, *kept the number of ids the chain kept, *cut_id the last kept
 * id of the order (logit descending, then id ascending); kept / cut_id / penalised may be NULL.
 * penalised[n_vocab]: the row after the penalties (bits of ids outside the history unchanged).
 * Every knob neutral runs the launch all the same (it keeps every id). */
int mio_hip_llm_debug_sample_chain(mio_hip_llm *m, const float *logits, const int32_t *history, int n_history,
                                   const mio_sampling *s, float temperature, uint64_t seed, int step, int32_t lo,
                                   int32_t hi, int32_t *token, int32_t *kept, int32_t *cut_id, float *penalised);

/* ---------------- MioCodec kernels, one launch each ----------------
 * Parity entry points of csrc/hip/codec_kernels.hip (csrc/testlib/debug_codec_capi.cpp). Every
 * pointer is host memory; a call uploads its operands, launches on the device's stream, waits
 * and downloads. Every output lives between two 256-byte guard zones, and guards and output
 * are filled with a sentinel (a quiet NaN with a payload) before the launch, so that a write
 * outside the buffer and an element no thread wrote both show: *guards_ok is 1 when both
 * zones still hold the sentinel, and an unwritten output element comes back as the sentinel.
 * (Outputs that are also inputs - the GEMM's C, an in-place row norm, a conv residual that
 * aliases Y - carry the caller's values between the guards instead.)
 * Arguments outside a kernel's documented preconditions are refused with MIO_ERR_INVALID. */

/* GemmArgs (csrc/hip/codec_kernels.h) field for field, plus the epilogue, the K-group count
 * (0: launch_gemm_f32 picks it and the tile order; 1, 2, 4: launch_gemm_f32_cfg(.., kg, 11))
 * and the row count of C (M rows, rows_out for the ConvT epilogues). */
typedef struct mio_debug_gemm {
    int a_seg, a_row_off, a_rows;
    int M, N, K;
    int ldc, c_rows;
    int f, trim, cout, rows_out;
    int m_major; /* passed through; both launchers overwrite it */
    int a_f16;
    int epi, kg;
} mio_debug_gemm;
/* A [a_rows][a_seg], B [N][K], C [c_rows][ldc] in/out; bias / aux / aux2 may be NULL where the
 * epilogue does not read them (per column: N values; ConvT epilogues: cout values). */
int mio_hip_debug_codec_gemm(mio_hip_device *d, const mio_debug_gemm *g, const float *A, const float *B,
                             float *C, const float *bias, const float *aux, const float *aux2,
                             int *guards_ok);
/* launch_conv_f16: xa [L][Cin] and w [Cout][taps*Cin] are f16 bit patterns, y [L][Cout].
 * resid_mode 0: no residual; 1: resid [L][Cout] is a buffer of its own; 2: the residual
 * aliases Y (y holds it on entry). */
int mio_hip_debug_codec_conv(mio_hip_device *d, const uint16_t *xa, int L, int Cin, int taps, int pad,
                             const uint16_t *w, int Cout, const float *bias, int resid_mode,
                             const float *resid, float *y, int *guards_ok);
/* launch_rownorm on x [M][D]; in_place: y is the x buffer (y still receives the result). */
int mio_hip_debug_codec_rownorm(mio_hip_device *d, const float *x, int M, int D, float eps, int mode,
                                const float *p0, const float *p1, int in_place, float *y, int *guards_ok);
/* launch_groupnorm_apply on x [L][C] (MIO_GN picks the pipeline): xa [L][C] f16 bit patterns. */
int mio_hip_debug_codec_groupnorm(mio_hip_device *d, const float *x, int L, int C, int G, float eps,
                                  const float *gamma, const float *beta, uint16_t *xa, int *guards_ok);
/* launch_band_attention: qkv [S][3*H*64], rope [S][32] (cos, sin) pairs, out [S][H*64]. */
int mio_hip_debug_codec_band_attention(mio_hip_device *d, const float *qkv, int S, int H, int window,
                                       const float *rope, float *out, int *guards_ok);
/* launch_cond_gemv: W [R][A], b [R], e [A] -> y [R]. */
int mio_hip_debug_codec_cond_gemv(mio_hip_device *d, const float *W, const float *b, const float *e, int R,
                                  int A, int e_f16, float *y, int *guards_ok);
/* launch_embed: table [n_rows][D], codes [T] in [0, n_rows) -> x [T][D]. */
int mio_hip_debug_codec_embed(mio_hip_device *d, const float *table, int n_rows, int D, const int32_t *codes,
                              int T, float *x, int *guards_ok);

/* ---------------- synthetic model files ----------------
 * No GGUF model files exist offline. These write files with the
 * reference's tensor names and KV keys (miocodec.cpp:448-481, 599-728;
 * create_voice_emb.py:125-129) filled with seeded N(0, s) weights.
 * preset 0 = MioCodec-25Hz-44.1kHz shapes, 1 = tiny test codec. */
int mio_synth_codec_gguf(const char *path, int preset, uint64_t seed);
int mio_synth_voice_gguf(const char *path, uint64_t seed);
/* Synthetic LLM (llama.cpp GGUF conventions, byte-level vocab + 12,800 speech tokens):
 * preset 0 tiny Q8_0, 1 tiny Q4_K_M, 2 "0.1B" Q8_0, 3 "1.7B" Q4_K_M, 4 "2.6B" Q8_0,
 * 5 tiny Q8_0 qwen2 with attn_{q,k,v}.bias, ... (csrc/testlib/synth.h lists all 19). */
int mio_synth_llm_gguf(const char *path, int preset, uint64_t seed);
/* The shape, arch and seed rule of `preset` written with the recipe `qtype`, in SynthLlmCfg's
 * numbering: 8 Q8_0, 15 Q4_K_M, 16 Q5_K_S, 17 Q5_K_M, 18 MOSTLY_Q6_K (every matrix Q6_K; rows
 * that are no multiple of 256 fall back to Q8_0), 2 Q4_0, 30 BF16; any other value is
 * MIO_ERR_INVALID. With the preset's own qtype the file equals mio_synth_llm_gguf's. */
int mio_synth_llm_gguf_as(const char *path, int preset, int qtype, uint64_t seed);
/* mio_synth_llm_gguf_as with sizes of the caller's: `preset`'s arch / rope / vocab / layer-kind
 * rules and head_dim, the recipe `qtype`, and n_embd, n_layer, n_head, n_head_kv, n_ff where not
 * 0 (0 keeps the preset's). The presets' own refusals (the Q5_K recipes' multiples of 256) hold;
 * row lengths that are no multiple of 32 and kv heads that do not divide the heads are
 * MIO_ERR_INVALID. */
int mio_synth_llm_gguf_shape(const char *path, int preset, int qtype, uint64_t seed, int n_embd, int n_layer,
                             int n_head, int n_head_kv, int n_ff);

#ifdef __cplusplus
}
#endif
#endif /* MIO_HIP_TEST_H */
