// A decoder layer's attention block as ONE launch of the single-token decode step (layers >= 1;
// llama_decode for one token, test-to-speech.cpp:178-185): RMSNorm + q|k|v matvec, the
// attention chunks and their merge, and the O projection + residual, which are k_attn_in,
// k_attention and k_attn_out's bodies as three workgroup roles of one grid:
//   [0, GW)                q|k|v producers (k_attn_in's body; rows stored write-through, then
//                          the rows each workgroup wrote per kv head added to that head's
//                          q|k|v row counter and, q rows, to its q row counter: qkv_word)
//   [GW, GW + n_act)       attention chunks (n_act = (pos / ATT_CHUNK + 1) * n_kv): K/V rows
//                          of the chunk loaded and staged in LDS first, then one lane waits
//                          for the head rows the chunk loads (the chunk that owns pos for the
//                          kv head's (G + 2) * hd rows, the others for its G * hd q rows
//                          only), which are loaded sc1 (attention_wg<..., WQ = true>); the
//                          owning chunk waits for the head's other chunks, merges
//                          (attn_merge_owner) and signals the O counters
//   [GW + n_act, + no)     O workgroups (o_consumer, as in k_att_o)
// Every consumer has a higher workgroup index than the producers it waits for, and producers
// never wait; chunk workgroups are chunk-major, so the owning chunk too has a higher index than
// the chunks it waits for, which wait for producers only: in-order dispatch makes progress
// whatever the residency (MI355X_MICROARCH
// "Persistent kernels": hand-offs inside a launch instead of a ~1.2-1.5 us boundary each).
// Layer 0 keeps k_attn_in (its sampler may end the step) + k_att_o. The counters are zeroed by
// the next launch, k_ffn_in. Instantiated for the shipped head shapes and weight types only
// (layer_att_supported); everything else runs the separate launches, whose math is the same.
#include "llm_attention.h"

#pragma clang fp contract(off)

namespace mio {
namespace {

template <int NP, int TQ, int TV, int SU, int HD, int G, bool DG>
__device__ __forceinline__ void qkv_producer(const float *x, const float *norm_w, const StepState *st, int K,
                                             const LlmDims &d, const QMat &wq, const QMat &wk, const QMat &wv, int g_qk,
                                             int GW, const LlmBuffers &b, unsigned long long entry_rt_,
                                             unsigned long long entry_cc_) {
    constexpr bool kDiag = DG;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const uint32_t dn = done_issue_st(st);
    XRegs<NP> xr;
    load_x(x, norm_w, K, xr);
    MIO_ENTRY_REST(MIO_PIN_QMAT(wq), MIO_PIN_QMAT(wk), MIO_PIN_QMAT(wv), "s"(b.att_cnt), "s"(b.qkv), "s"(d.eps));
    MIO_ENTRY_COMMIT(b);
    zero_ffn_counters(b.att_cnt);
    const int o1 = wq.rows, o2 = wq.rows + wk.rows;
    const Smem s = carve(smem, K);
    auto put = [&](int row, float v) { st1_sc1(b.qkv, (uint32_t)row * 4, v); };
    Frag ga[Cfg<NP, SU>::U], gb[Cfg<NP, SU>::U];
    int lo, hi, ra, rb;
    const int bid = blockIdx.x;
    if (bid < g_qk) {
        wave_range(o2, lo, hi, bid, g_qk);
        ra = o2 * bid / g_qk, rb = o2 * (bid + 1) / g_qk;
        load_first<TQ, NP, 1, SU, MIO_SMALL_AUX>(wq, wk, lo, hi, ga, gb, o1);
        x_after_weights(xr);
        if (done_now(dn)) return;
        MIO_TL_MARK1(b);
        rmsnorm_quant(xr, K, d.eps, akind(TQ), s, MIO_TL_DIAGSLOT(b));
        MIO_TL_MARK(b, 2);
        stream_rows_lanes<TQ, NP, 1, SU, MIO_SMALL_AUX>(wq, wk, lo, hi, ga, gb, s.a, [&](int row, float v, float) {
            put(row, v);
        }, o1);
    } else {
        const int bv = bid - g_qk, gv = GW - g_qk;
        wave_range(wv.rows, lo, hi, bv, gv);
        ra = o2 + wv.rows * bv / gv, rb = o2 + wv.rows * (bv + 1) / gv;
        load_first<TV, NP, 1, SU, MIO_SMALL_AUX>(wv, wv, lo, hi, ga, gb);
        x_after_weights(xr);
        if (done_now(dn)) return;
        MIO_TL_MARK1(b);
        rmsnorm_quant(xr, K, d.eps, akind(TV), s, MIO_TL_DIAGSLOT(b));
        MIO_TL_MARK(b, 2);
        stream_rows_lanes<TV, NP, 1, SU, MIO_SMALL_AUX>(wv, wv, lo, hi, ga, gb, s.a, [&](int row, float v, float) {
            put(o2 + row, v);
        });
    }
    // every row of the workgroup written through, then per (kv head, q or k|v) ONE add of the
    // workgroup's row count to the head's q|k|v word and, for q rows, one more to its q word
    // (runs of equal keys over rows ra .. rb - 1 <= 64, host-checked): key 2 h for head h's q
    // rows, 2 h + 1 for its k and its v row
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (MIO_TIDX < 64) {
        const int i = MIO_TIDX, r = ra + i;
        auto head_of = [&](int rr) {
            return rr < o1 ? 2 * (rr / (HD * G)) : 2 * ((rr < o2 ? rr - o1 : rr - o2) / HD) + 1;
        };
        const bool ok = r < rb;
        const int h = ok ? head_of(r) : -1;
        const bool start = ok && (i == 0 || head_of(r - 1) != h);
        const uint64_t m = __ballot(start);
        if (start) {
            const uint64_t nx = i < 63 ? m >> (i + 1) : 0;
            const int end = nx ? i + 1 + __builtin_ctzll(nx) : rb - ra;
            if (!(h & 1))
                __hip_atomic_fetch_add((__attribute__((address_space(1))) int *)qkv_word(b.att_cnt, h >> 1, false),
                                       end - i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add((__attribute__((address_space(1))) int *)qkv_word(b.att_cnt, h >> 1, true), end - i,
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// Entry pack (llm_device.h "kernel entry"): x, the attention norm weight, the state, K = n_embd,
// the role split (g_qk, GW) and n_kv ((pos / ATT_CHUNK + 1) * n_kv attention workgroups); the
// earlier list follows (its norm_w, g_qk and GW are the pack's now and stay unnamed).
template <int NP, int TQ, int TV, int SU, int HD, int G, int TO, int SUO, bool DG>
__global__ __launch_bounds__(MT) void k_layer_att(const float *x, const float *norm_w, StepState *st, int K, int g_qk,
                                                  int GW, int n_kv, LlmDims d, const float *, QMat wq, QMat wk, QMat wv,
                                                  int, int, const float *q_norm, const float *k_norm, const float *bqkv,
                                                  _Float16 *kc, _Float16 *vc, QMat wo, LlmBuffers b) {
    constexpr bool kDiag = DG;
    MIO_ENTRY_STAMPS();
    const int bid = blockIdx.x;
    if (bid < GW) {
        qkv_producer<NP, TQ, TV, SU, HD, G, DG>(x, norm_w, st, K, d, wq, wk, wv, g_qk, GW, b, entry_rt_, entry_cc_);
    } else {
        // pos and the end-token flag through the pack (state_issue): beside the batch, not behind it
        const StateRegs sr = state_issue(st);
        MIO_ENTRY_REST("s"(kc), "s"(vc), "s"(d.n_ctx), "s"(b.qkv), "s"(b.rope), "s"(q_norm), "s"(k_norm), "s"(b.part),
                       "s"(d.max_splits), "s"(bqkv), "s"(b.att), "s"(b.att_cnt), MIO_PIN_QMAT(wo), "s"(d.n_wg),
                       "s"(b.x));
        MIO_ENTRY_COMMIT(b);
        zero_ffn_counters(b.att_cnt);
        const int pos = state_pos(sr, d.n_ctx);
        if (state_done(sr)) return;  // the producers return too: nobody signals, nobody waits
        const int ab = bid - GW, n_act = (pos / ATT_CHUNK + 1) * n_kv;
        if (ab < n_act) {
            if (MIO_TIDX >= AttCfg<HD>::NT) return;  // whole waves; s_barrier counts the live ones
            if (!attention_wg<HD, G, DG, true, true>(d, q_norm, k_norm, bqkv, kc, vc, b, false, ab / n_kv, ab % n_kv, pos,
                                               b.att_cnt + kRdyOff))
                return;
        } else {
            const int no = matvec_grid_n(d.n_wg, wo.rows), ob = ab - n_act;
            if (ob >= no) return;
            o_consumer<1, TO, SUO, DG>(d, wo, wo.k, b, ob, no);
        }
    }
    MIO_TL_END(b);
    MIO_TRACE(b, 15);
}

// the instantiated (np, q|k type, v type, su, hd, G, o type, o su): 1.7B Q4_K_M (v Q4_K or
// Q6_K), Q5_K_M / Q5_K_S (q|k, o Q5_K, v Q5_K or Q6_K), Q6_K (every matrix) and BF16, 0.1B Q8_0,
// 2.6B Q8_0 (and the LFM2-2.6B attention layers) and Q6_K; last, the 1.7B shape as Q3_K_S (every
// matrix Q3_K), Q3_K_M (v Q4_K or Q5_K, o Q4_K) and Q3_K_L (v, o Q5_K)
#define MIO_LAYER_ATT_SHAPES(X)   \
    X(1, GGML_Q4_K, GGML_Q4_K, 2, 128, 2, GGML_Q4_K, 1)              \
    X(1, GGML_Q4_K, GGML_Q6_K, 2, 128, 2, GGML_Q4_K, 1)              \
    X(1, GGML_Q5_K, GGML_Q5_K, 2, 128, 2, GGML_Q5_K, 1)              \
    X(1, GGML_Q5_K, GGML_Q6_K, 2, 128, 2, GGML_Q5_K, 1)              \
    X(1, GGML_Q6_K, GGML_Q6_K, 2, 128, 2, GGML_Q6_K, 1)              \
    X(1, GGML_BF16, GGML_BF16, 2, 128, 2, GGML_BF16, 1)              \
    X(1, GGML_Q8_0, GGML_Q8_0, 1, 64, 3, GGML_Q8_0, 1)               \
    X(1, GGML_Q8_0, GGML_Q8_0, 2, 64, 4, GGML_Q8_0, 1)               \
    X(1, GGML_Q6_K, GGML_Q6_K, 2, 64, 4, GGML_Q6_K, 1)               \
    X(1, GGML_Q3_K, GGML_Q3_K, 2, 128, 2, GGML_Q3_K, 1)              \
    X(1, GGML_Q3_K, GGML_Q4_K, 2, 128, 2, GGML_Q4_K, 1)              \
    X(1, GGML_Q3_K, GGML_Q5_K, 2, 128, 2, GGML_Q4_K, 1)              \
    X(1, GGML_Q3_K, GGML_Q5_K, 2, 128, 2, GGML_Q5_K, 1)

struct Shape {
    int np, tq, tv, su, hd, g, to, suo;
    int GW, g_qk;
};

Shape shape_of(const LlmDims &d, const LayerW &L) {
    Shape s{};
    attn_in_grid(d, L, s.GW, s.g_qk);
    s.np = pick_np(d.n_embd);
    s.tq = L.wq.type, s.tv = L.wv.type, s.to = L.wo.type;
    s.su = pick_su(std::max(max_wave_units(L.wq.rows + L.wk.rows, s.g_qk, s.np, 1),
                            max_wave_units(L.wv.rows, s.GW - s.g_qk, s.np, 1)),
                   s.np);
    s.suo = pick_su(max_wave_units(L.wo.rows, matvec_grid(d, L.wo.rows), pick_np(L.wo.k), 1), pick_np(L.wo.k));
    s.hd = d.hd, s.g = d.n_head / d.n_kv;
    if (pick_np(L.wo.k) != 1) s.suo = -1;
    return s;
}

template <bool DG>
bool launch(const LlmDims &d, const LayerW &L, _Float16 *kc, _Float16 *vc, const LlmBuffers &b, hipStream_t st,
            bool dry) {
    const Shape s = shape_of(d, L);
    const int rows = L.wq.rows + L.wk.rows + L.wv.rows;
    // the producer's per-head signal covers <= 64 rows per workgroup
    if ((L.wq.rows + L.wk.rows + s.g_qk - 1) / s.g_qk > 64 || (L.wv.rows + s.GW - s.g_qk - 1) / (s.GW - s.g_qk) > 64 ||
        d.n_kv > kQkvMax || rows != (d.n_head + 2 * d.n_kv) * d.hd || L.conv)
        return false;
    const int grid = s.GW + d.max_splits * d.n_kv + matvec_grid(d, L.wo.rows);
    const size_t lds = std::max(matvec_lds(d.n_embd), matvec_lds(L.wo.k));
    bool found = false;
#define MIO_LA_CASE(NP, TQ, TV, SU, HD, G, TO, SUO)                                                                   \
    if (!found && s.np == NP && s.tq == TQ && s.tv == TV && s.su == SU && s.hd == HD && s.g == G && s.to == TO &&   \
        s.suo == SUO) {                                                                                                \
        found = true;                                                                                                  \
        if (!dry)                                                                                                      \
            hipLaunchKernelGGL((k_layer_att<NP, TQ, TV, SU, HD, G, TO, SUO, DG>), dim3(grid), dim3(MT), lds, st, b.x, \
                               L.attn_norm, b.st, d.n_embd, s.g_qk, s.GW, d.n_kv, d, L.attn_norm, L.wq, L.wk, L.wv,    \
                               s.g_qk, s.GW, L.q_norm, L.k_norm, L.bqkv, kc, vc, L.wo, b);                             \
    }
    MIO_LAYER_ATT_SHAPES(MIO_LA_CASE)
#undef MIO_LA_CASE
    return found;
}

}  // namespace

bool layer_att_supported(const LlmDims &d, const LayerW &L) {
    return launch<false>(d, L, nullptr, nullptr, LlmBuffers{}, nullptr, true);
}

void launch_layer_att(const LlmDims &d, const LayerW &L, _Float16 *kc, _Float16 *vc, const LlmBuffers &b, bool dg,
                      hipStream_t s) {
    if (dg)
        launch<true>(d, L, kc, vc, b, s, false);
    else
        launch<false>(d, L, kc, vc, b, s, false);
}

}  // namespace mio
