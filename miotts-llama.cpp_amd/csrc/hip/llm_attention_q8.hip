// Attention on the Q8_0 K/V cache (KvQ8, llm_kernels.h; row format and helpers: llm_kv_q8.h): the
// counterparts of k_attention (llm_kernels.hip) and of k_pf_rope / k_pf_attention / k_bt_attention
// (llm_prefill.hip) for a handle loaded with kv type GGML_Q8_0.
//
//   k_attention_q8     the single-stream step's attention launch (between k_attn_in and k_attn_out)
//   k_pf_rope_q8       chunked prefill: q heads prepared in place, k / v rows quantized into the planes
//   k_pf_attention_q8  chunked prefill: every row read back from the planes
//   k_bt_attention_q8  the batched step: one token per sequence
//
// A chunk workgroup loads int8 codes and f16 scales (0.53 x the F16 rows' bytes), dequantizes in
// registers into the same swizzled f16 LDS images, and runs attend_chunk_mfma and the merge of the
// F16 cache unchanged. The wave that prepares the new k | v row quantizes it (per-32 amax by lane
// exchanges), stores codes and scales, and stages the DEQUANTIZED row: the step that appends a row,
// every later step, the batched step and the prefill all attend to the same f16 values, so their
// outputs are equal bit for bit as on the F16 cache.
// The four planes are kernel arguments of their own; LlmDims, LlmBuffers and PrefillBuffers are
// the F16 launches'.
#include "llm_kv_q8.h"

namespace mio {
namespace {

// Shared by k_attention_q8 and k_bt_attention_q8: the (chunk t0, kv head) workgroup's q heads as
// f16 and its K / V images at position pos, from the raw q|k|v row qkv. kq .. vs: the kv head's
// planes of the token's sequence. The owner of pos (the chunk holding it) appends row pos.
// attend(qh, img) runs once both are visible.
template <int HD, int G, class F>
__device__ __forceinline__ void chunk_q8(const LlmDims &d, const float *qkv, const float *q_norm, const float *k_norm,
                                         const float *bqkv, const float2 *rope, int8_t *kq, _Float16 *ks, int8_t *vq,
                                         _Float16 *vs, int kvh, int t0, int pos, F &&attend) {
    using C = AttCfg<HD>;
    using A = AttM<HD>;
    constexpr int PER = HD / 64;
    static_assert(C::NT == A::NT, "attention workgroup size");
    __shared__ float qs[G][HD];
    __shared__ float knew[HD], vnew[HD];
    __shared__ __attribute__((aligned(16))) char img[2 * A::IMG];
    __shared__ __attribute__((aligned(16))) _Float16 qh[G][HD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool owner = pos < t0 + ATT_CHUNK;
    // the loads of each wave's first head go out before its K/V units (as k_attention)
    auto head_src = [&](int hh, HeadIn<HD> &in) {
        const bool isk = hh == G;
        const size_t so = isk ? (size_t)(d.n_head + kvh) * HD : (size_t)(kvh * G + hh) * HD;
        const size_t vo = (size_t)(d.n_head + d.n_kv + kvh) * HD;
        head_load<HD>(qkv + so, bqkv ? bqkv + so : nullptr, isk ? k_norm : q_norm, rope, d, in,
                      isk ? qkv + vo : nullptr, isk && bqkv ? bqkv + vo : nullptr);
    };
    HeadIn<HD> hin;
    if (wave < G + (owner ? 1 : 0)) head_src(wave, hin);
    KvQ8Regs<HD> kr;
    kv_issue_q8<HD>(kq, ks, vq, vs, t0, pos, kr);  // row pos is staged from LDS below
    for (int hh = wave; hh < G + (owner ? 1 : 0); hh += C::NW) {
        const bool isk = hh == G;
        if (hh != wave) head_src(hh, hin);
        head_prep<HD>(hin, d, isk ? knew : qs[hh]);
        if (isk) {
            float kx[PER], vx[PER];
#pragma unroll
            for (int i = 0; i < PER; ++i) kx[i] = knew[lane + 64 * i], vx[i] = f16r(hin.vv[i]);
            q8_quant_row<HD>(kx, kq + (size_t)pos * HD, ks + (size_t)pos * (HD / 32));
            q8_quant_row<HD>(vx, vq + (size_t)pos * HD, vs + (size_t)pos * (HD / 32));
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
#pragma unroll
            for (int i = 0; i < PER; ++i) knew[lane + 64 * i] = kx[i], vnew[lane + 64 * i] = vx[i];
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            kv_stage_row<HD>(knew, vnew, pos - t0, img, img + A::IMG);
        } else {
            q_to_f16<HD>(qs[hh], qh[hh]);
        }
    }
    kv_stage_q8<HD>(kr, owner ? pos - t0 : -1, img, img + A::IMG);
    lds_barrier();
    attend(qh, img);
}

// One workgroup per (chunk of ATT_CHUNK positions, kv head), grid (max_splits, n_kv): k_attention
// on the Q8_0 planes of the layer. The partial records, the tickets and b.att are k_attention's.
template <int HD, int G, bool DG>
__global__ __launch_bounds__(AttCfg<HD>::NT) void k_attention_q8(LlmDims d, const float *q_norm, const float *k_norm,
                                                                 const float *bqkv, int8_t *kq, _Float16 *ks,
                                                                 int8_t *vq, _Float16 *vs, LlmBuffers b) {
    constexpr bool kDiag = DG;
    using C = AttCfg<HD>;
    MIO_TRACE(b, 0);
    MIO_TL_BEGIN(b);
    // as k_attention: every argument the workgroup uses arrives with the round trip that fetches b.st
    asm volatile("" ::"s"(kq), "s"(ks), "s"(vq), "s"(vs), "s"(d.n_ctx), "s"(b.qkv), "s"(b.rope), "s"(q_norm),
                 "s"(k_norm), "s"(b.part), "s"(d.max_splits), "s"(bqkv), "s"(b.att), "s"(b.att_cnt));
    const int pos = cur_pos(b.st, d);
    const int ch = blockIdx.x, kvh = blockIdx.y, t0 = ch * ATT_CHUNK;
    if (t0 > pos || b.st->done != 0) return;
    const size_t ro = (size_t)kvh * d.n_ctx;  // the kv head's first row
    chunk_q8<HD, G>(d, b.qkv, q_norm, k_norm, bqkv, b.rope + (size_t)pos * (HD / 2), kq + ro * HD, ks + ro * (HD / 32),
                    vq + ro * HD, vs + ro * (HD / 32), kvh, t0, pos, [&](const _Float16(*qh)[HD], const char *img) {
                        MIO_TL_MARK(b, 2);
                        const uint32_t gs = (uint32_t)(d.max_splits * C::REC), head0 = (uint32_t)(kvh * G) * gs;
                        attend_chunk_mfma<HD, G>(qh, img, img + AttM<HD>::IMG, t0, pos, d.scale,
                                                 b.part + head0 + (uint32_t)ch * C::REC, gs, DG ? b.trace : nullptr);
                        attn_merge_last<HD, G>(b.part, head0, gs, pos / ATT_CHUNK + 1, b.att_cnt + kvh,
                                               b.att + (size_t)kvh * G * HD, -1, {}, 0, nullptr,
                                               (kDiag && b.tl) ? MIO_TL_SLOT(b) : nullptr);
                    });
    MIO_TL_END(b);
    MIO_TRACE(b, 15);
}

// One wave per (head, token): k_pf_rope with the k | v row quantized into the planes.
template <int HD>
__global__ __launch_bounds__(64) void k_pf_rope_q8(LlmDims d, const float *q_norm, const float *k_norm,
                                                   const float *bqkv, int8_t *kq, _Float16 *ks, int8_t *vq,
                                                   _Float16 *vs, PrefillBuffers pb) {
    constexpr int PER = HD / 64;
    __shared__ float row[HD];
    const int hh = blockIdx.x, t = blockIdx.y, lane = threadIdx.x;
    const int pos = pb.pos[t * pb.pos_stride];
    const int QD = (d.n_head + 2 * d.n_kv) * HD;
    const bool isk = hh >= d.n_head;
    const int kvh = hh - d.n_head;
    float *src = pb.qkv + (size_t)t * QD + (size_t)hh * HD;
    float vx[PER];
    if (isk) {
        const size_t vo = (size_t)(d.n_head + d.n_kv + kvh) * HD;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            vx[i] = pb.qkv[(size_t)t * QD + vo + lane + 64 * i];
            if (bqkv) vx[i] = vx[i] + bqkv[vo + lane + 64 * i];
            vx[i] = f16r(vx[i]);
        }
    }
    prep_head<HD>(src, bqkv ? bqkv + (size_t)hh * HD : nullptr, isk ? k_norm : q_norm,
                  pb.rope + (size_t)pos * (HD / 2), d, row);
    if (!isk) {
#pragma unroll
        for (int i = 0; i < PER; ++i) src[lane + 64 * i] = row[lane + 64 * i];
    } else {
        // rows (of HD codes / HD / 32 scales) in front of this one: sequence, kv head, position
        const size_t ro = (size_t)pb.seq[t * pb.seq_stride] * (pb.seq_kv / HD) + (size_t)kvh * d.n_ctx + pos;
        float kx[PER];
#pragma unroll
        for (int i = 0; i < PER; ++i) kx[i] = row[lane + 64 * i];
        q8_quant_row<HD>(kx, kq + ro * HD, ks + ro * (HD / 32));
        q8_quant_row<HD>(vx, vq + ro * HD, vs + ro * (HD / 32));
    }
}

// One workgroup per (chunk, kv head, token), grid (n_kv * nt, chunks): k_pf_attention with every
// row, the token's own included (k_pf_rope_q8 wrote it), read from the planes.
template <int HD, int G>
__global__ __launch_bounds__(AttCfg<HD>::NT) void k_pf_attention_q8(LlmDims d, const int8_t *kq, const _Float16 *ks,
                                                                    const int8_t *vq, const _Float16 *vs,
                                                                    PrefillBuffers pb, int att_q) {
    using C = AttCfg<HD>;
    using A = AttM<HD>;
    const int kvh = blockIdx.x % d.n_kv, t = blockIdx.x / d.n_kv, ch = blockIdx.y;
    const int pos = pb.pos[t * pb.pos_stride];
    const int t0 = ch * ATT_CHUNK;
    if (t0 > pos) return;
    const size_t ro = (size_t)pb.seq[t * pb.seq_stride] * (pb.seq_kv / HD) + (size_t)kvh * d.n_ctx;
    const int QD = (d.n_head + 2 * d.n_kv) * HD;
    const float *qsrc = pb.qkv + (size_t)t * QD + (size_t)kvh * G * HD;
    __shared__ __attribute__((aligned(16))) char img[2 * A::IMG];
    __shared__ __attribute__((aligned(16))) _Float16 qh[G][HD];
    KvQ8Regs<HD> kr;
    kv_issue_q8<HD>(kq + ro * HD, ks + ro * (HD / 32), vq + ro * HD, vs + ro * (HD / 32), t0, pos, kr, true);
    for (int e = threadIdx.x; e < G * HD; e += C::NT) qh[e / HD][e % HD] = (_Float16)qsrc[e];
    kv_stage_q8<HD>(kr, -1, img, img + A::IMG);
    lds_barrier();
    attend_and_merge<HD, G>(d, qh, img, t0, pos, ch, t, kvh, pb, att_q);
}

// One workgroup per (chunk, kv head, token), one token per sequence: k_bt_attention on the planes.
template <int HD, int G>
__global__ __launch_bounds__(AttCfg<HD>::NT) void k_bt_attention_q8(LlmDims d, const float *q_norm,
                                                                    const float *k_norm, const float *bqkv,
                                                                    int8_t *kq, _Float16 *ks, int8_t *vq, _Float16 *vs,
                                                                    PrefillBuffers pb, int att_q) {
    const int kvh = blockIdx.x % d.n_kv, t = blockIdx.x / d.n_kv, ch = blockIdx.y;
    const int pos = pb.pos[t * pb.pos_stride];
    const int t0 = ch * ATT_CHUNK;
    // a frozen stream's attention is skipped (k_bt_attention: pb.pos points at its StepState)
    static_assert(offsetof(StepState, done) - offsetof(StepState, pos) == 3 * sizeof(int), "StepState layout");
    if (t0 > pos || pb.pos[t * pb.pos_stride + 3]) return;
    const size_t ro = (size_t)pb.seq[t * pb.seq_stride] * (pb.seq_kv / HD) + (size_t)kvh * d.n_ctx;
    chunk_q8<HD, G>(d, pb.qkv + (size_t)t * (d.n_head + 2 * d.n_kv) * HD, q_norm, k_norm, bqkv,
                    pb.rope + (size_t)pos * (HD / 2), kq + ro * HD, ks + ro * (HD / 32), vq + ro * HD,
                    vs + ro * (HD / 32), kvh, t0, pos, [&](const _Float16(*qh)[HD], const char *img) {
                        attend_and_merge<HD, G>(d, qh, img, t0, pos, ch, t, kvh, pb, att_q);
                    });
}

// f.template operator()<G>() for the query heads per kv head the loader accepts
template <class F>
void dispatch_g(int G, F &&f) {
    switch (G) {
        case 1: return f.template operator()<1>();
        case 2: return f.template operator()<2>();
        case 3: return f.template operator()<3>();
        case 4: return f.template operator()<4>();
        case 8: return f.template operator()<8>();
        default: return;
    }
}

}  // namespace

void launch_attention_q8(const LlmDims &d, const LayerW &L, const KvQ8 &kv, const LlmBuffers &b, hipStream_t s) {
    const dim3 grid(d.max_splits, d.n_kv);
    dispatch_hd(d.hd, [&]<int HD>() {
        dispatch_g(d.n_head / d.n_kv, [&]<int G>() {
            // diagnostic instantiation only when a trace / timeline buffer is attached
            auto k = (b.tl || b.trace) ? k_attention_q8<HD, G, true> : k_attention_q8<HD, G, false>;
            hipLaunchKernelGGL(k, grid, dim3(AttCfg<HD>::NT), 0, s, d, L.q_norm, L.k_norm, L.bqkv, kv.kq, kv.ks, kv.vq,
                               kv.vs, b);
        });
    });
}

void launch_mt_attention_q8(const LlmDims &d, const LayerW &L, const KvQ8 &kv, const PrefillBuffers &pb, int nt,
                            int n_chunks, bool decode, int att_q, hipStream_t s) {
    const dim3 grid(d.n_kv * nt, n_chunks);
    dispatch_hd(d.hd, [&]<int HD>() {
        dispatch_g(d.n_head / d.n_kv, [&]<int G>() {
            const dim3 block(AttCfg<HD>::NT);
            if (decode) {
                hipLaunchKernelGGL((k_bt_attention_q8<HD, G>), grid, block, 0, s, d, L.q_norm, L.k_norm, L.bqkv, kv.kq,
                                   kv.ks, kv.vq, kv.vs, pb, att_q);
                return;
            }
            hipLaunchKernelGGL((k_pf_rope_q8<HD>), dim3(d.n_head + d.n_kv, nt), dim3(64), 0, s, d, L.q_norm, L.k_norm,
                               L.bqkv, kv.kq, kv.ks, kv.vq, kv.vs, pb);
            hipLaunchKernelGGL((k_pf_attention_q8<HD, G>), grid, block, 0, s, d, kv.kq, kv.ks, kv.vq, kv.vs, pb, att_q);
        });
    });
}

}  // namespace mio
