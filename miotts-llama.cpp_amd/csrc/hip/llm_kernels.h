// Launch interface of the LLM decode-step kernels (csrc/hip/llm_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "weight_types.h"

namespace mio {

// attention positions per chunk (one attention workgroup), = LlmDims::split. Every path
// (decode step, batched decode, prefill) uses the same chunks and the same merge, so their
// results are bit-identical. MIO_ATT_CHUNK: A/B builds (32, 64 or 128); 64 by default
// (profiles/r04_att_chunk_ab.txt: 1.7B decode 0.823 / 0.773 / 0.775 ms per token at 32 / 64 / 128).
#ifndef MIO_ATT_CHUNK
#define MIO_ATT_CHUNK 64
#endif
constexpr int kAttChunk = MIO_ATT_CHUNK;
// step timeline (diagnostic): workgroup slots per launch (larger grids wrap)
constexpr int kTlSlots = 2048;
static_assert(kAttChunk == 32 || kAttChunk == 64 || kAttChunk == 128, "attention chunk");

// One quantized matrix in the split layout (csrc/weight_types.h), rows x k.
struct QMat {
    int type;  // GgmlType, one of kWeightTypes (weight_types.h)
    int rows, k;
    const uint8_t *p0, *p1, *p2, *p3;
};

// Rows [r0, r0 + n) of q as a matrix of its own (every split-layout stream is row-major).
inline QMat qmat_rows(const QMat &q, int r0, int n) {
    QMat v = q;
    v.rows = n;
    v.p0 = q.p0 + plane_row_bytes(q.type, q.k, 0) * r0, v.p1 = q.p1 + plane_row_bytes(q.type, q.k, 1) * r0;
    v.p2 = q.p2 + plane_row_bytes(q.type, q.k, 2) * r0, v.p3 = q.p3 + plane_row_bytes(q.type, q.k, 3) * r0;
    return v;
}

// Device-resident decode state (read by every kernel of a step; advanced by the sampler),
// so one captured hipGraph replays every token without host involvement.
// The sampler of step t runs inside step t+1's first launch (layer 0 attn_in) and the flush
// launch after the last step: `pending` = the lm_head partials of step `step` are not sampled
// yet, so the token being decoded sits at min(pos + pending, n_ctx - 1) (cur_pos) until
// layer 0's ffn_in folds pending into pos / step.
struct StepState {
    int pos;      // position of the last sampled token (cur_pos: of the token being decoded)
    int step;     // step counter (sampler RNG counter, output slot)
    int token;    // token being decoded
    int done;     // set once an end token was sampled
    int pending;  // 1: lm_head partials of this step await the sampler
};

struct SampleCfg {
    float temp;
    uint32_t seed_lo, seed_hi;
    int lo, hi;          // sampled ids restricted to [lo, hi)
    int eos0, eos1;      // end tokens (-1 = none)
    const int *force;    // force[step] >= 0: next token is forced (prompt prefill), or null
    int n_force;
    int *out_tokens;     // [max_steps] sampled/forced next token per step
    int max_steps;
    int *host_done;      // mapped host word set to 1 with StepState.done (null: none)
    // the sampler chain (k_sample_chain, llm_sample_chain.hip); read by that launch alone, which
    // is in the step only when a knob is off its neutral value
    int top_k;                // <= 0 or >= the window: off
    float top_p, min_p;       // >= 1: off; <= 0: off
    float repeat_penalty, frequency_penalty, presence_penalty;  // 1, 0, 0: off
    int repeat_last_n;        // history length, 0..kChainHistMax (0: no penalties)
    int first_step;           // the first sampled step: out_tokens[first_step .. step) is the history
};
constexpr int kChainHistMax = 256;

// lfm2 gated short conv: kernel width (shortconv.l_cache) and the ring of bx values kept per
// layer (slot p & 3 holds position p; positions p-2, p-1 are read while p is written)
constexpr int kConvL = 3;
constexpr int kConvSlots = 4;

struct LayerW {
    const float *attn_norm, *q_norm, *k_norm, *ffn_norm;
    const float *bqkv;  // [(H + 2 Hkv) hd] q|k|v biases (qwen2 attn_{q,k,v}.bias), or null
    QMat wq, wk, wv, wo, gate, up, down;
    // lfm2 short-conv layer (conv != 0; wq..wo unused): in_proj [3 n_embd][n_embd] -> B | C | X,
    // depthwise taps conv_w [n_embd][kConvL] f32, out_proj [n_embd][n_embd]
    int conv;
    QMat in_proj, out_proj;
    const float *conv_w;
};

struct LlmDims {
    int n_embd, n_head, n_kv, hd, n_ff, n_vocab, n_ctx;
    float eps, scale;
    int neox, qk_norm;
    int split;        // attention positions per chunk (kAttChunk)
    int max_splits;
    int n_wg;         // streaming-matvec workgroups (one per CU)
    int n_layer;
};

struct LlmBuffers {
    float *x;          // [n_embd] residual stream
    float *qkv;        // [(H + 2 Hkv) hd]
    float *h;          // [n_ff] ffn activation
    float *logits;     // [n_vocab]
    float *part;       // [H][max_splits][hd + 4] attention chunk partials {O, m, l}
    float *att;        // [H * hd] attention output (chunks merged by one chunk workgroup per kv head)
    int *att_cnt;      // [Hkv] chunk arrival tickets (0 between launches); the fused launches'
                       // counters and wait-timeout flag at kRdyOff.. (kAttCntInts in all)
    float *smp;        // sampler partials [2 * n_lm_blocks]
    const float2 *rope;  // [n_ctx][hd/2] (cos, sin)
    StepState *st;
    const SampleCfg *cfg;       // sampling configuration (device-resident: graphs never re-capture)
    unsigned long long *trace;  // optional: per-kernel checkpoint timestamps (workgroup 0, thread 0)
    unsigned long long *tl;     // optional: step timeline {min start, max end} per launch (s_memrealtime)
    int seq;                    // launch index within the step (timeline slot)
    float *ring;   // lfm2: [n_layer][kConvSlots][n_embd] short-conv inputs bx by position
};

// Batched prompt prefill (csrc/hip/llm_prefill.hip): up to kPrefillB prompt tokens per chunk
// go through every layer with ONE weight pass per launch (the prefill llama_decode of
// test-to-speech.cpp:132-148); K/V rows are written, no logits are produced. 128 holds the
// chat-template prompts of the benchmarks (≈70 tokens) in one chunk: a 64-token chunk left
// their last few tokens to a second, dot4 weight pass (+1.5 ms per 68-token prompt).
// Memory: the chunk's attention partials (PrefillBuffers.part) are kPrefillB x n_head x
// ceil(n_ctx / kAttChunk) x (hd + 4) floats: at the default 64-position chunks 35 MB for the 1.7B
// model at n_ctx 2048 and 554 MB at the 32768 maximum (of 288 GB); the merged outputs pb.att
// add kPrefillB x n_head x hd floats (1 MB) and the tickets pb.att_cnt kPrefillB x n_kv ints.
constexpr int kPrefillB = 128;
// The same multi-token layers run the batched decode step of up to kBatchMax utterances.
constexpr int kBatchMax = 16;

// The batched decode step of B independent utterances runs the same layers (one token of
// each per step, weights streamed once for all of them).
struct PrefillBuffers {
    float *x;            // [kPrefillB][n_embd] residual streams
    float *qkv;          // [kPrefillB][(H + 2 Hkv) hd]; q rows are RoPE'd in place (lfm2 conv
                         // layers: [kPrefillB][3 n_embd] B | C | X rows)
    float *h;            // [kPrefillB][n_ff]
    float *part;         // [kPrefillB][H][max_splits][hd + 4] attention chunk partials
    float *att;          // [kPrefillB][H * hd] attention outputs (merged in the attention launch)
    int *att_cnt;        // [kPrefillB][Hkv] chunk arrival tickets (0 between launches)
    const float2 *rope;  // [n_ctx][hd/2]
    const int *tokens;   // device token ids (embedded token t of a chunk at tokens[p0 + t])
    const int *pos;      // position of token t: pos[t * pos_stride] (device-resident)
    const int *seq;      // sequence (KV cache) of token t: seq[t * seq_stride]
    int pos_stride, seq_stride;
    size_t seq_kv;       // K (and V) cache elements per sequence: [seq][layer][kv head][n_ctx][hd]
    float *ring;         // lfm2 short-conv rings [seq][n_layer][kConvSlots][n_embd], or null
    size_t seq_ring;     // ring elements per sequence
    char *act;           // [kPrefillB] quantized activation records of the next matvec
    int *qcnt;           // batched decode, in-launch quantization (launch_mmq_q): 2 sets of 8
                         // counter shards 64 ints apart, then the wait-timeout flag (kQcntFlag)
};
constexpr int kQcntFlag = 1024, kQcntInts = kQcntFlag + 64;
// bytes of the act records (pb.act) for K up to k_max (BF16 weights: pass prefill_rec_k)
size_t prefill_act_bytes(int k_max);
// K of the act record layout for a weight type (2K for BF16: K bf16 values)
int prefill_rec_k(int K, int type);

// One chunk of nt <= kPrefillB tokens (ids at tokens[p0 + t], positions/sequences from
// pb.pos / pb.seq) through every layer: embedding, K/V rows, residual streams in pb.x.
// n_chunks = attention chunks to sweep (>= max position / kAttChunk + 1).
void launch_prefill_chunk(const LlmDims &d, const LayerW *layers, int n_layer, _Float16 *kcache,
                          _Float16 *vcache, const QMat &tok_embd, const PrefillBuffers &pb, int p0, int nt,
                          int n_chunks, hipStream_t s);

// Batched decode of B <= kBatchMax streams: per stream b, state st[b], sampling cfg[b]
// (cfg[b].out_tokens[step] = where the token of that step goes: the output region of the utterance
// the stream decodes, QueueBuffers.out), logits [B][n_vocab], sampler partials smp [B][lm blocks][2];
// the residual streams are pb.x[b].
struct BatchBuffers {
    StepState *st;
    const SampleCfg *cfg;
    float *logits;
    float *smp;
};
// One decode step of all B sequences: every layer with one weight pass per launch, the
// lm_head for all B, (chain: the sampler chain launch,) then per-sequence sampling + next
// embedding + state advance.
void launch_batch_step(const LlmDims &d, const LayerW *layers, int n_layer, _Float16 *kcache, _Float16 *vcache,
                       const float *out_norm, const QMat &lm, const QMat &tok_embd, const PrefillBuffers &pb,
                       const BatchBuffers &bb, int B, bool chain, hipStream_t s);
// B streams fit one batched step (B <= kBatchMax and the lm_head's LDS for its weight type)
bool batch_supported(const LlmDims &d, int B, int lm_type);

// The utterance queue on the batched decode (mio_hip_llm_generate_queue, and _generate_batch with
// a slot per utterance): what an admission reads on the device, uploaded once per call.
struct QueueUtt {
    int tok_off;  // its prompt in QueueBuffers.tokens
    int P;        // prompt length - 1: positions [0, P) are prefilled, decoding starts at P
    int budget;   // sampled tokens at most (max_steps = P + budget)
    int out_off;  // its output region in QueueBuffers.out: step s goes to out[out_off + s - P]
    uint32_t seed_lo, seed_hi;
};
struct QueueBuffers {
    const int *tokens;    // every prompt of the queue, concatenated
    const QueueUtt *utt;  // [N]
    int *out;             // n_ctx ints of slack (out_off - P stays inside), then the output regions
    int *host_done;       // [N] mapped host words, one per utterance (SampleCfg.host_done)
    int *ptok, *ppos, *pseq;  // the flattened prefill lists the admission's chunks read
};
// The admissions of one graph boundary: utterance utt[j] into slot slot[j], its P prompt
// positions at flat[j] of the flattened lists.
struct QueueRefill {
    int n;
    int slot[kBatchMax], utt[kBatchMax], flat[kBatchMax];
};
// Before the prefill chunks: the list entries, and (lfm2) the slots' short-conv rings zeroed.
void launch_queue_refill(const PrefillBuffers &pb, const QueueBuffers &q, const QueueRefill &r, hipStream_t s);
// After them: the admitted slots' StepState and SampleCfg (base + the table), and the next input
// of all B slots embedded into pb.x.
void launch_queue_admit(const LlmDims &d, const QMat &tok_embd, const PrefillBuffers &pb, const BatchBuffers &bb,
                        SampleCfg *cfg, const SampleCfg &base, const QueueBuffers &q, const QueueRefill &r, int B,
                        hipStream_t s);

// The launches of a decode step. The numbers are an interface and stay as they are: bench.py,
// tools/, the tests and the callers of mio_hip_llm_step_kinds / _time_kernel / _trace_kernel
// pass them as int (the C ABI keeps int). 5 was the final norm, now inside lm_head.
enum StepKind : int {
    kAttnIn = 0,      // RMSNorm + q|k|v (+ layer 0: the previous step's sampler)
    kAttention = 1,   // attention chunks + merge
    kAttnOut = 2,     // O projection + residual
    kFfnIn = 3,       // RMSNorm + gate|up (+ layer 0: pos / step advance)
    kFfnDown = 4,     // down projection + residual
    kLmHead = 6,      // final norm + lm_head + sampler partials
    kSample = 7,      // flush sampler (after the last step)
    kConvIn = 8,      // lfm2 short-conv layer: RMSNorm + in_proj, in place of 0
    kConvOut = 9,     // lfm2 short-conv layer: gated conv + out_proj, in place of 1 + 2
    kAttO = 10,       // k_att_o: 1 + 2
    kLayerAtt = 11,   // k_layer_att: 0 + 1 + 2
    kFfn = 12,        // k_ffn: 3 + 4
                      // 13 is unused (it was the whole layer as one launch, removed)
    kSampleChain = 14,  // k_sample_chain: penalties + top-k / top-p / min-p + draw (after 6, chain on only)
    kStepKindEnd = 15,
};
// What every launch of a model's step shares (the host builds it once per model).
struct StepCtx {
    LlmDims dims;
    const LayerW *layers;
    _Float16 *kc, *vc;
    const float *out_norm;
    QMat lm, tok;
};
// The sampler chain launch: stream t (one workgroup each, B of them) reads logits + t * stride,
// st[t], cfg[t] and rewrites its nblk sampling partials smp + t * nblk * 2. dbg (parity entry,
// or null): {kept count, id at the cut, 1} per stream; keep: the penalised row stays in logits.
struct ChainArgs {
    float *logits;
    size_t stride;
    const StepState *st;
    const SampleCfg *cfg;
    float *smp;
    int nblk;
    int *dbg;
    int keep;
};
void launch_sample_chain(const ChainArgs &a, int B, hipStream_t s);
// Launch kernel `which` of a decode step (of layer il where it is a layer's) on stream s.
void launch_step_kernel(StepKind which, const StepCtx &c, int il, const LlmBuffers &b, hipStream_t s);
// Embedding of `token` (row of token_embd) -> b.x, and state reset to (pos, token).
void launch_embed_token(const LlmDims &d, const QMat &tok_embd, const LlmBuffers &b, hipStream_t s);
int lm_head_blocks(const LlmDims &d);
// workgroups of a streaming matvec over `rows` rows (at least 8 rows per workgroup, at most
// one workgroup per CU); passes of 2048 weights for K. Kernels recompute it from their
// arguments instead of reading gridDim (an implicit kernel argument, one more scalar-load
// round trip before the first weight load).
__host__ __device__ inline int matvec_grid_n(int n_wg, int rows) {
    int g = rows / 8;
    g = g < n_wg ? g : n_wg;
    return g < 2 ? 2 : g;
}
int matvec_grid(const LlmDims &d, int rows);
// the fused attention + O launch (launch_step_kernel which = 10) exists for this head shape
bool att_o_supported(int hd, int G);
// the whole attention block of layer L as one launch (llm_layer_att.hip, which = 11) exists for
// its shapes and weight types
bool layer_att_supported(const LlmDims &d, const LayerW &L);
// the FFN pair of layer L as one launch (k_ffn, which = 12) exists for its weight types
bool ffn_fused_supported(const LlmDims &d, const LayerW &L);
void launch_layer_att(const LlmDims &d, const LayerW &L, _Float16 *kc, _Float16 *vc, const LlmBuffers &b, bool dg,
                      hipStream_t s);
// k_att_o's merge counters in LlmBuffers.att_cnt: kRdyShards words kRdyStride ints (256 B)
// apart from int kRdyOff on (one per XCD: an O workgroup polls shard blockIdx % 8, so no word
// has more than 1/8 of the pollers; MI355X_MICROARCH "dequeue": one word saturates near 88
// accesses per us), then the wait-timeout flag. Needs n_kv <= kRdyOff.
// Then three polled words per kv head (at most kQkvMax heads, kQkvStride ints apart, the words
// of a head 256 B apart): k_layer_att's q row counter (+ 0; the head's G * hd q rows) and q|k|v
// row counter (+ kAllSub; all its (G + 2) * hd rows: a q row is counted in both), and the chunk
// arrival word of the fused launches (+ kArrSub: attn_merge_owner; the owning chunk zeroes it).
constexpr int kRdyOff = 64, kRdyShards = 8, kRdyStride = 64;
constexpr int kRdyFlag = kRdyOff + kRdyShards * kRdyStride;
constexpr int kQkvOff = kRdyFlag + 64, kAllSub = 64, kArrSub = 128, kQkvStride = 192, kQkvMax = 64;
// Then the fused FFN launch's h counters (k_ffn, which = 12), two levels, every word kFfnStride
// ints apart: kFfnShards arrival shards (gate|up workgroup b adds 1 to shard b % 8: <= 32 adds
// per word at 256 producers; the price list's fan-in on one word is 3.6-4.5 us), then
// kFfnShards ready replicas (the producer whose shard add returns the shard's last count adds 1
// to every replica; a down workgroup polls replica b % 8 until all shards are in: <= 32 pollers
// per word). Zeroed by the launch after k_ffn (the next layer's attn_in / layer_att, lm_head).
constexpr int kFfnOff = kQkvOff + kQkvStride * kQkvMax, kFfnShards = 8, kFfnStride = 64;
constexpr int kFfnRdy = kFfnOff + kFfnShards * kFfnStride;
constexpr int kAttCntInts = kFfnRdy + kFfnShards * kFfnStride;
int pick_np(int K);
size_t matvec_lds(int K);
// units (row passes) of the busiest wave of a matvec over `rows` rows on `grid` workgroups,
// and the single-group size that covers them (0 = streaming groups)
int max_wave_units(int rows, int grid, int np, int nm);
int pick_su(int units, int np);
// Layer il's first launch (llm_attn_in.hip): RMSNorm + q|k|v matvec (+ layer 0: the
// previous step's sampler).
void launch_attn_in(const LlmDims &d, const LayerW &L, int il, const QMat &tok_embd, const LlmBuffers &b, bool dg,
                    hipStream_t s);
// y = W x with x re-quantized to the vec_dot_type (parity test of the matvec kernels); with
// up: y = silu(W x) * (up x), the gate|up launch's row pairs and epilogue.
void launch_debug_matvec(const QMat &W, const QMat *up, const float *x, float *y, int n_wg, hipStream_t s);
// The same on the single-group row stream of su units per wave over `grid` workgroups (the form
// the decode step launches); false: no such instantiation, or a wave would own more than su units.
bool launch_debug_matvec_group(const QMat &W, const QMat *up, const float *x, float *y, int su, int grid,
                               hipStream_t s);
// The decode prologue's activation quantizer for weight type `type` on x[K] (RMSNorm with w when
// given; sc1: the hand-off load path): the LDS record, debug_act_record_bytes(K) bytes, to out.
size_t debug_act_record_bytes(int K);
void launch_debug_act_quant(int type, const float *x, const float *w, int K, float eps, bool sc1, void *out,
                            hipStream_t s);
// y[t][rows] = W x[t] for nt tokens on the int8-MFMA multi-token matmul (act: scratch of
// nt * debug_act_bytes(W.k) bytes); mode 0 store, 1 y += W x, 2 y = silu(W x) * (up x).
size_t debug_act_bytes(int K);
void launch_debug_mmq(const QMat &W, const QMat &up, int mode, const float *x, int nt, char *act, float *y,
                      hipStream_t s);

}  // namespace mio
