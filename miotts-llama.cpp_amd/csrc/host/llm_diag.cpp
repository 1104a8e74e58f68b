// Parity-test entry points and profiling diagnostics of the LLM runner (see llm.h,
// llm_model.h; include/mio_hip.h, include/mio_hip_test.h). No product path calls these.
#include <algorithm>
#include <cstring>

#include "gguf.h"
#include "llm_model.h"
#include "quant.h"

extern "C" int mio_hip_llm_step_kinds(const mio_hip_llm *m, int *kinds, int cap, int *n) {
    MIO_REQUIRE(m && n, MIO_ERR_INVALID, "llm_step_kinds: null");
    const std::vector<mio::StepKind> k = step_kinds(m);
    *n = (int)k.size();
    MIO_REQUIRE(!kinds || cap >= (int)k.size(), MIO_ERR_INVALID, "llm_step_kinds: need %d slots", (int)k.size());
    if (kinds) std::copy(k.begin(), k.end(), kinds);
    return MIO_OK;
}

// lfm2 short-conv ring of layer il, [kConvSlots][n_embd] (bx of position p in slot p & 3;
// parity tests). get: copied out; set: copied in.
extern "C" int mio_hip_llm_conv_ring(mio_hip_llm *m, int il, float *ring, int set) {
    MIO_REQUIRE(m && ring && il >= 0 && il < m->n_layer && m->layers[il].conv && m->buf.ring, MIO_ERR_INVALID,
                "llm_conv_ring: layer %d is not a short-conv layer", il);
    int rc = mio::bind(m->d);
    if (rc) return rc;
    const size_t n = (size_t)mio::kConvSlots * m->dims.n_embd;
    float *dr = m->buf.ring + (size_t)il * n;
    hipStream_t s = m->d->stream;
    if (set)
        MIO_HIP_CHECK(hipMemcpyAsync(dr, ring, n * 4, hipMemcpyHostToDevice, s));
    else
        MIO_HIP_CHECK(hipMemcpyAsync(ring, dr, n * 4, hipMemcpyDeviceToHost, s));
    MIO_HIP_CHECK(hipStreamSynchronize(s));
    return MIO_OK;
}

// One decode step like mio_hip_llm_eval, launched kernel by kernel, with the residual stream
// captured before layer 0 (the embedding) and after every layer: x_layers[(n_layer + 1) *
// n_embd] (parity tests: the oracle re-runs each layer on the GPU's input).
extern "C" int mio_hip_llm_eval_layers(mio_hip_llm *m, int32_t token, int pos, float *x_layers, float *logits) {
    MIO_REQUIRE(m && x_layers && token >= 0 && token < m->dims.n_vocab && pos >= 0 && pos < m->dims.n_ctx,
                MIO_ERR_INVALID, "llm_eval_layers: bad args");
    int rc = mio::bind(m->d);
    if (rc) return rc;
    if ((rc = put_cfg(m, greedy_cfg(m))) || (rc = ensure_graph(m))) return rc;
    const int zero = 0;
    hipStream_t s = m->d->stream;
    const size_t D = (size_t)m->dims.n_embd;
    MIO_HIP_CHECK(hipMemcpyAsync(m->d_force, &zero, 4, hipMemcpyHostToDevice, s));
    if ((rc = set_state(m, pos, token))) return rc;
    if (!m->d_layers) {
        void *p = nullptr;
        MIO_HIP_CHECK(hipMalloc(&p, (m->n_layer + 1) * D * 4));
        m->allocs.push_back(p);
        m->d_layers = (float *)p;
    }
    float *dx = m->d_layers;
    MIO_HIP_CHECK(hipMemcpyAsync(dx, m->buf.x, D * 4, hipMemcpyDeviceToDevice, s));
    mio::StepKind w[kLayerKindsMax];
    for (int il = 0; il < m->n_layer; ++il) {
        for (int i = 0, n = layer_kinds(m, il, w); i < n; ++i) mio::launch_step_kernel(w[i], m->ctx(), il, m->buf, s);
        MIO_HIP_CHECK(hipMemcpyAsync(dx + (il + 1) * D, m->buf.x, D * 4, hipMemcpyDeviceToDevice, s));
    }
    mio::launch_step_kernel(mio::kLmHead, m->ctx(), 0, m->buf, s);
    MIO_HIP_CHECK(hipGetLastError());
    MIO_HIP_CHECK(hipMemcpyAsync(x_layers, dx, (m->n_layer + 1) * D * 4, hipMemcpyDeviceToHost, s));
    if (logits)
        MIO_HIP_CHECK(hipMemcpyAsync(logits, m->buf.logits, (size_t)m->dims.n_vocab * 4, hipMemcpyDeviceToHost, s));
    if ((rc = flush_sample(m))) return rc;
    MIO_HIP_CHECK(hipStreamSynchronize(s));
    return check_handoff(m);
}

// F16 K / V cache rows [0, n_pos) of layer il as [n_kv][n_pos][head_dim] (parity tests).
extern "C" int mio_hip_llm_kv_rows(mio_hip_llm *m, int il, int n_pos, uint16_t *k, uint16_t *v) {
    MIO_REQUIRE(m && k && v && il >= 0 && il < m->n_layer && n_pos >= 0 && n_pos <= m->dims.n_ctx, MIO_ERR_INVALID,
                "llm_kv_rows: bad args");
    int rc = mio::bind(m->d);
    if (rc) return rc;
    const mio::LlmDims &D = m->dims;
    hipStream_t s = m->d->stream;
    for (int h = 0; h < D.n_kv; ++h) {
        const size_t src = (((size_t)il * D.n_kv + h) * D.n_ctx) * D.hd, dst = (size_t)h * n_pos * D.hd;
        MIO_HIP_CHECK(hipMemcpyAsync(k + dst, m->kc + src, (size_t)n_pos * D.hd * 2, hipMemcpyDeviceToHost, s));
        MIO_HIP_CHECK(hipMemcpyAsync(v + dst, m->vc + src, (size_t)n_pos * D.hd * 2, hipMemcpyDeviceToHost, s));
    }
    MIO_HIP_CHECK(hipStreamSynchronize(s));
    return MIO_OK;
}

// The inverse of mio_hip_llm_kv_rows (parity tests): rows [n_kv][n_pos][head_dim] into cache
// positions [p0, p0 + n_pos) of layer il.
int mio::llm_set_kv_rows(mio_hip_llm *m, int il, int p0, int n_pos, const uint16_t *k, const uint16_t *v) {
    MIO_REQUIRE(m && k && v && il >= 0 && il < m->n_layer && p0 >= 0 && n_pos >= 0 && p0 <= m->dims.n_ctx &&
                    n_pos <= m->dims.n_ctx - p0,
                MIO_ERR_INVALID, "llm_set_kv_rows: bad args");
    int rc = mio::bind(m->d);
    if (rc) return rc;
    const mio::LlmDims &D = m->dims;
    hipStream_t s = m->d->stream;
    for (int h = 0; h < D.n_kv && n_pos > 0; ++h) {
        const size_t dst = (((size_t)il * D.n_kv + h) * D.n_ctx + p0) * D.hd, src = (size_t)h * n_pos * D.hd;
        MIO_HIP_CHECK(hipMemcpyAsync(m->kc + dst, k + src, (size_t)n_pos * D.hd * 2, hipMemcpyHostToDevice, s));
        MIO_HIP_CHECK(hipMemcpyAsync(m->vc + dst, v + src, (size_t)n_pos * D.hd * 2, hipMemcpyHostToDevice, s));
    }
    MIO_HIP_CHECK(hipStreamSynchronize(s));
    return MIO_OK;
}

// The polled words of the attention hand-offs per kv head (tests of the counters' hygiene):
// words[3 h + 0 .. 2] = head h's q row counter, q|k|v row counter and chunk arrival word. All are
// 0 between steps. reset: reset_tickets first.
int mio::llm_handoff_words(mio_hip_llm *m, int reset, int32_t *words) {
    MIO_REQUIRE(m && words && m->dims.n_kv <= mio::kQkvMax, MIO_ERR_INVALID, "llm_handoff_words: bad args");
    int rc = mio::bind(m->d);
    if (rc) return rc;
    if (reset && (rc = reset_tickets(m))) return rc;
    hipStream_t s = m->d->stream;
    const int sub[3] = {0, mio::kAllSub, mio::kArrSub};
    for (int h = 0; h < m->dims.n_kv; ++h)
        for (int j = 0; j < 3; ++j)
            MIO_HIP_CHECK(hipMemcpyAsync(words + 3 * h + j, m->buf.att_cnt + mio::kQkvOff + mio::kQkvStride * h + sub[j],
                                         sizeof(int), hipMemcpyDeviceToHost, s));
    MIO_HIP_CHECK(hipStreamSynchronize(s));
    return MIO_OK;
}

// One attention launch on an injected q|k|v row (parity tests): the state is set to pos, the
// row replaces buf.qkv, launch_step_kernel(which) of layer il runs alone, and buf.att comes
// back. kAttO also runs the O workgroups (buf.x += W_o att, on token 0's embedding).
int mio::llm_debug_attention(mio_hip_llm *m, int il, int pos, int which, const float *qkv, float *att) {
    MIO_REQUIRE(m && qkv && att && il >= 0 && il < m->n_layer && pos >= 0 && pos < m->dims.n_ctx, MIO_ERR_INVALID,
                "llm_debug_attention: bad args");
    MIO_REQUIRE(!m->layers[il].conv, MIO_ERR_INVALID, "llm_debug_attention: layer %d is a short-conv layer", il);
    const mio::LlmDims &D = m->dims;
    MIO_REQUIRE(which == kAttention || which == kAttO, MIO_ERR_UNSUPPORTED, "llm_debug_attention: which %d (%d or %d)",
                which, kAttention, kAttO);
    // whatever MIO_ATT_FUSE_O says: the launch itself is what the test is about
    MIO_REQUIRE(which == kAttention || (D.n_kv <= mio::kRdyOff && mio::att_o_supported(D.hd, D.n_head / D.n_kv) &&
                                        m->layers[il].wo.k <= 2048),  // k_att_o: one 2048-weight pass of W_o
                MIO_ERR_UNSUPPORTED, "llm_debug_attention: no attention + O launch for this shape");
    int rc = mio::bind(m->d);
    if (rc) return rc;
    hipStream_t s = m->d->stream;
    if ((rc = set_state(m, pos, 0))) return rc;  // tickets and merge counters zeroed, state at pos
    const size_t n_qkv = (size_t)(D.n_head + 2 * D.n_kv) * D.hd, n_att = (size_t)D.n_head * D.hd;
    MIO_HIP_CHECK(hipMemcpyAsync(m->buf.qkv, qkv, n_qkv * 4, hipMemcpyHostToDevice, s));
    mio::launch_step_kernel((StepKind)which, m->ctx(), il, m->buf, s);
    MIO_HIP_CHECK(hipGetLastError());
    MIO_HIP_CHECK(hipMemcpyAsync(att, m->buf.att, n_att * 4, hipMemcpyDeviceToHost, s));
    // the O workgroups' wait flag, read here whatever MIO_ATT_FUSE_O says (check_handoff follows it)
    int flag = 0;
    MIO_HIP_CHECK(hipMemcpyAsync(&flag, m->buf.att_cnt + mio::kRdyFlag, sizeof(int), hipMemcpyDeviceToHost, s));
    MIO_HIP_CHECK(hipStreamSynchronize(s));
    if (flag) {
        MIO_HIP_CHECK(hipMemsetAsync(m->buf.att_cnt + mio::kRdyFlag, 0, sizeof(int), s));
        mio::set_error("llm_debug_attention: the attention -> O hand-off wait timed out");
        return MIO_ERR_HIP;
    }
    return check_handoff(m);
}

// One sampler chain launch on an injected logits row (parity tests): the row replaces
// buf.logits, `history` (the tokens the run is taken to have sampled so far, oldest first)
// fills the token ring in front of `step`, the lm_head partials are set to "no id", the chain
// launch and the flush sampler run, and the state's token comes back with the launch's kept
// count and cut id (0 / -1 where the launch left the step to the plain sampler: empty window).
int mio::llm_debug_sample_chain(mio_hip_llm *m, const float *logits, const int32_t *history, int n_history,
                                const SamplingParams &sp, int step, int32_t *token, int32_t *kept, int32_t *cut_id,
                                float *penalised) {
    MIO_REQUIRE(m && logits && token && n_history >= 0 && (history || !n_history), MIO_ERR_INVALID,
                "llm_debug_sample_chain: null argument");
    MIO_REQUIRE(step >= n_history && step < m->max_steps, MIO_ERR_INVALID,
                "llm_debug_sample_chain: step %d outside [n_history %d, %d)", step, n_history, m->max_steps);
    int rc = check_chain(sp, "llm_debug_sample_chain");
    if (rc || (rc = mio::bind(m->d))) return rc;
    hipStream_t s = m->d->stream;
    const size_t V = (size_t)m->dims.n_vocab;
    const int nblk = mio::lm_head_blocks(m->dims);
    mio::SampleCfg c = sample_cfg(m, sp, sp.seed, m->d_tokens, nullptr, m->max_steps);
    c.first_step = step - n_history;
    if ((rc = put_cfg(m, c))) return rc;
    const mio::StepState st{0, step, 0, 0, 1};
    std::vector<float> none((size_t)nblk * 2);
    const int imax = INT_MAX;
    for (int i = 0; i < nblk; ++i) none[2 * i] = -INFINITY, std::memcpy(&none[2 * i + 1], &imax, 4);
    int *dbg = nullptr;
    MIO_HIP_CHECK(hipMalloc(&dbg, 3 * sizeof(int)));
    auto run = [&]() -> int {
        MIO_HIP_CHECK(hipMemsetAsync(dbg, 0, 3 * sizeof(int), s));
        MIO_HIP_CHECK(hipMemcpyAsync(m->buf.st, &st, sizeof(st), hipMemcpyHostToDevice, s));
        MIO_HIP_CHECK(hipMemcpyAsync(m->buf.logits, logits, V * 4, hipMemcpyHostToDevice, s));
        MIO_HIP_CHECK(hipMemcpyAsync(m->buf.smp, none.data(), none.size() * 4, hipMemcpyHostToDevice, s));
        if (n_history)
            MIO_HIP_CHECK(hipMemcpyAsync(m->d_tokens + c.first_step, history, (size_t)n_history * 4,
                                         hipMemcpyHostToDevice, s));
        mio::launch_sample_chain(mio::ChainArgs{m->buf.logits, 0, m->buf.st, m->d_cfg, m->buf.smp, nblk, dbg,
                                                penalised ? 1 : 0}, 1, s);
        MIO_HIP_CHECK(hipGetLastError());
        if (penalised) MIO_HIP_CHECK(hipMemcpyAsync(penalised, m->buf.logits, V * 4, hipMemcpyDeviceToHost, s));
        if ((rc = flush_sample(m))) return rc;
        int d3[3] = {0, 0, 0};
        mio::StepState out{};
        MIO_HIP_CHECK(hipMemcpyAsync(d3, dbg, sizeof(d3), hipMemcpyDeviceToHost, s));
        MIO_HIP_CHECK(hipMemcpyAsync(&out, m->buf.st, sizeof(out), hipMemcpyDeviceToHost, s));
        MIO_HIP_CHECK(hipStreamSynchronize(s));
        *token = out.token;
        if (kept) *kept = d3[2] ? d3[0] : 0;
        if (cut_id) *cut_id = d3[2] ? d3[1] : -1;
        return MIO_OK;
    };
    rc = run();
    hipFree(dbg);
    return rc;
}

namespace {

// The layer a diagnostic launch of `kind` runs on: the first layer at or after n_layer / 2
// (wrapping) that can run it (kind_in_layer), or -1.
int kernel_layer(const mio_hip_llm *m, mio::StepKind kind) {
    for (int i = 0; i < m->n_layer; ++i) {
        const int il = (m->n_layer / 2 + i) % m->n_layer;
        if (kind_in_layer(m, kind, il)) return il;
    }
    return -1;
}

// Shared prologue of time_kernel / trace_kernel (`who` names the caller in the error text):
// the model has run, `which` is a launch this model has a layer for (*il), the device is bound.
int diag_prepare(mio_hip_llm *m, int which, const char *who, int *il) {
    MIO_REQUIRE(m && m->graph, MIO_ERR_INVALID, "%s: run generate/eval first", who);
    MIO_REQUIRE(which >= 0 && which < mio::kStepKindEnd, MIO_ERR_INVALID, "%s: which %d", who, which);
    MIO_REQUIRE(which != mio::kSampleChain, MIO_ERR_INVALID,
                "%s: the sampler chain (kind %d) is not a launch the diagnostics run", who, which);
    *il = kernel_layer(m, (mio::StepKind)which);
    MIO_REQUIRE(*il >= 0, MIO_ERR_INVALID, "%s: the model has no layer with kernel %d", who, which);
    return mio::bind(m->d);
}

// Decode state a diagnostic launch may change, saved at entry and put back on exit: the
// StepState (k_lm_head sets `pending`, layer 0's k_ffn_in folds it into pos) and the
// residual x (attn_out / ffn_down / conv_out add into it; after a flush it holds the next
// token's embedding). The other buffers a launch writes are rewritten by the next real step
// before anything reads them: the K/V row and the short-conv ring slot of cur_pos (the
// owner stores them first), q|k|v, h, the chunk partials and the lm_head partials (the same
// inputs give the same values).
struct DiagStateGuard {
    mio_hip_llm *m;
    mio::StepState st{};
    mio::Scratch<float> x;
    int rc = MIO_OK;
    explicit DiagStateGuard(mio_hip_llm *mm) : m(mm) {
        const size_t xb = (size_t)m->dims.n_embd * sizeof(float);
        if (hipStreamSynchronize(m->d->stream) != hipSuccess ||
            hipMemcpy(&st, m->buf.st, sizeof(st), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMalloc((void **)x.put(), xb) != hipSuccess ||
            hipMemcpy(x, m->buf.x, xb, hipMemcpyDeviceToDevice) != hipSuccess) {
            mio::set_error("llm diagnostic: saving the decode state failed");
            rc = MIO_ERR_HIP;
        }
    }
    ~DiagStateGuard() {
        hipStreamSynchronize(m->d->stream);
        if (x) hipMemcpy(m->buf.x, x, (size_t)m->dims.n_embd * sizeof(float), hipMemcpyDeviceToDevice);
        if (rc == MIO_OK) hipMemcpy(m->buf.st, &st, sizeof(st), hipMemcpyHostToDevice);
    }
};

// Algorithmic HBM bytes of one launch of `kind` on layer L with the decode state at position
// pos: weights of the matrices it streams + activations. A value handed over inside a fused
// launch (q|k|v, h, x: written and read back by its own workgroups) is counted once each
// way, exactly as for the launches it replaces, so a fused launch's bytes are the sum of its
// parts.
uint64_t kind_bytes(const mio_hip_llm *m, mio::StepKind kind, const mio::LayerW &L, uint64_t pos) {
    const mio::LlmDims &D = m->dims;
    // the bytes the split layout streams (weight_types.h), as mio_hip_llm_weight_bytes counts them
    auto qbytes = [](const mio::QMat &q) { return (uint64_t)mio::row_bytes(q.type, q.k) * (uint64_t)q.rows; };
    const uint64_t nch = pos / mio::kAttChunk + 1, qkv = (uint64_t)(D.n_head + 2 * D.n_kv) * D.hd;
    // chunk partial records {O, m, l}: written by the chunk workgroups, read back by the
    // merging one (attn_merge_last / attn_merge_owner), which writes the n_head * hd outputs
    const uint64_t part = 4ull * D.n_head * nch * (D.hd + 2);
    // x in + the q|k|v weights; q|k|v out only where another launch reads it
    const uint64_t attn_in_bytes = qbytes(L.wq) + qbytes(L.wk) + qbytes(L.wv) + 4ull * D.n_embd;
    // attention: F16 K and V rows of positions 0..pos (the row at pos is written, the rest
    // read) + q|k|v in + RoPE pair + partial records out and back + outputs
    const uint64_t att_bytes =
        2ull * 2 * D.n_kv * D.hd * (pos + 1) + 4ull * qkv + 8ull * (D.hd / 2) + 2 * part + 4ull * D.n_head * D.hd;
    const uint64_t o_bytes = qbytes(L.wo) + 4ull * D.n_head * D.hd + 4ull * D.n_embd * 2;
    const uint64_t ffn_in_bytes = qbytes(L.gate) + qbytes(L.up) + 4ull * (D.n_embd * 2 + D.n_ff);
    const uint64_t ffn_down_bytes = qbytes(L.down) + 4ull * (D.n_ff + 2 * D.n_embd);
    const uint64_t lm_bytes = qbytes(m->lm) + 4ull * D.n_vocab;
    const uint64_t conv_in_bytes = qbytes(L.in_proj) + 4ull * D.n_embd * 4;
    // B | C | X in, taps, the two window rows, this position's bx (one workgroup), x in / out
    const uint64_t conv_out_bytes = qbytes(L.out_proj) + 4ull * D.n_embd * (3 + mio::kConvL + 2 + 1 + 2);
    const uint64_t layer_att_bytes = attn_in_bytes + att_bytes + o_bytes, ffn_bytes = ffn_in_bytes + ffn_down_bytes;
    switch (kind) {
        case mio::kAttnIn: return attn_in_bytes + 4ull * qkv;
        case mio::kAttention: return att_bytes;
        case mio::kAttnOut: return o_bytes;
        case mio::kAttO: return att_bytes + o_bytes;
        case mio::kLayerAtt: return layer_att_bytes;
        case mio::kFfnIn: return ffn_in_bytes;
        case mio::kFfnDown: return ffn_down_bytes;
        case mio::kFfn: return ffn_bytes;
        case mio::kLmHead: return lm_bytes;
        case mio::kConvIn: return conv_in_bytes;
        case mio::kConvOut: return conv_out_bytes;
        default: return 0;
    }
}

}  // namespace

// Live timing of one kernel of the decode step (bench.py roofline): launches kernel `which`
// (a StepKind other than the flush sampler) of layer kernel_layer() `iters` times on the
// runner's stream between HIP events (as a replayed graph, below), with the buffers and device state
// left by the last generate/eval. Returns the mean duration and the algorithmic HBM bytes of
// one launch (kind_bytes, at the decode state's current pos).
extern "C" int mio_hip_llm_time_kernel(mio_hip_llm *m, int which, int iters, float *avg_ms, uint64_t *bytes) {
    MIO_REQUIRE(avg_ms && bytes && iters > 0, MIO_ERR_INVALID, "llm_time_kernel: bad args");
    MIO_REQUIRE(which != mio::kSample, MIO_ERR_INVALID, "llm_time_kernel: which %d", which);
    int il = 0;
    if (int rc = diag_prepare(m, which, "llm_time_kernel", &il)) return rc;
    const mio::StepKind kind = (mio::StepKind)which;
    // attention reads the K/V rows of positions <= pos of the current decode state; the
    // decode state is put back on exit (DiagStateGuard)
    DiagStateGuard guard(m);
    if (guard.rc) return guard.rc;
    const mio::StepState &st = guard.st;
    // the position the attention kernels work at (cur_pos: pos + pending)
    const uint64_t pos = (uint64_t)std::max(0, std::min(st.pos + st.pending, m->dims.n_ctx - 1));
    mio::Event e0, e1;
    MIO_HIP_CHECK(hipEventCreate(e0.put()));
    MIO_HIP_CHECK(hipEventCreate(e1.put()));
    hipStream_t s = m->d->stream;
    // The fused launches' hand-off counters are zeroed by the launch after them in a step: here
    // a memset does it before every launch, and a loop of the memsets alone is timed and
    // subtracted. Both loops are captured as hipGraphs and replayed: GPU-paced, +-0.3 % between
    // reps and within 5 % of the rocprof means of a real step, where eagerly issued loops were
    // partly host-paced (k_layer_att moved 11.7-14.9 us between runs of one tree;
    // profiles/r06/time_kernel_modes.txt).
    const bool fused = kind >= mio::kAttO;
    auto launch = [&](bool kernel) -> int {
        if (int rc = fused ? reset_rdy(m, s) : MIO_OK) return rc;
        if (kernel) mio::launch_step_kernel(kind, m->ctx(), il, m->buf, s);
        return MIO_OK;
    };
    auto timed = [&](bool kernel, float &ms) -> int {
        mio::GraphExec ge;
        auto launches = [&]() -> int {
            int rc = MIO_OK;
            for (int i = 0; i < iters && rc == MIO_OK; ++i) rc = launch(kernel);
            return rc;
        };
        if (int rc = mio::capture_graph(s, launches, ge.put())) return rc;
        MIO_HIP_CHECK(hipGraphLaunch(ge, s));  // warm replay
        MIO_HIP_CHECK(hipEventRecord(e0, s));
        MIO_HIP_CHECK(hipGraphLaunch(ge, s));
        MIO_HIP_CHECK(hipEventRecord(e1, s));
        MIO_HIP_CHECK(hipEventSynchronize(e1));
        MIO_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
        return MIO_OK;
    };
    if (int rc = launch(true)) return rc;  // warm
    float ms = 0, ms_ref = 0;
    if (int rc = timed(true, ms)) return rc;
    if (fused) {
        if (int rc = timed(false, ms_ref)) return rc;
        ms = std::max(0.0f, ms - ms_ref);
    }
    *avg_ms = ms / iters;
    *bytes = kind_bytes(m, kind, m->layers[il], pos);
    return MIO_OK;
}

// Runs kernel `which` (any StepKind time_kernel accepts, or the flush sampler) once, after a
// warm launch, with checkpoint tracing on; out[0..31]: s_memtime at checkpoints 0..15 of
// workgroup 0 / thread 0, s_memrealtime (100 MHz) at checkpoints 0 and 15 in out[16] /
// out[31]. Diagnostic only.
extern "C" int mio_hip_llm_trace_kernel(mio_hip_llm *m, int which, uint64_t *out) {
    MIO_REQUIRE(out, MIO_ERR_INVALID, "llm_trace_kernel: bad args");
    int il = 0;
    if (int rc = diag_prepare(m, which, "llm_trace_kernel", &il)) return rc;
    const mio::StepKind kind = (mio::StepKind)which;
    hipStream_t s = m->d->stream;
    DiagStateGuard guard(m);  // the decode state is put back on exit
    if (guard.rc) return guard.rc;
    mio::Scratch<unsigned long long> dt;
    MIO_HIP_CHECK(hipMalloc((void **)dt.put(), 32 * sizeof(unsigned long long)));
    MIO_HIP_CHECK(hipMemsetAsync(dt, 0, 32 * sizeof(unsigned long long), s));
    const bool fused = kind >= mio::kAttO;
    if (int rc = fused ? reset_rdy(m, s) : MIO_OK) return rc;
    mio::launch_step_kernel(kind, m->ctx(), il, m->buf, s);
    // evict L2 / MALL so the traced launch streams its weights from HBM as in a real step
    mio::Scratch<void> flush;
    const size_t flush_bytes = (size_t)1 << 30;
    if (hipMalloc(flush.put(), flush_bytes) == hipSuccess) {
        hipMemsetAsync(flush, 1, flush_bytes, s);
        hipMemsetAsync(flush, 2, flush_bytes, s);
    }
    mio::LlmBuffers tb = m->buf;
    tb.trace = dt;
    if (int rc = fused ? reset_rdy(m, s) : MIO_OK) return rc;
    mio::launch_step_kernel(kind, m->ctx(), il, tb, s);
    MIO_HIP_CHECK(hipMemcpyAsync(out, dt, 32 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    MIO_HIP_CHECK(hipStreamSynchronize(s));
    return MIO_OK;
}

// Diagnostic: captures one decode step as a graph with the step timeline on, replays it
// (advancing the decode state by 3 steps: reset/eval afterwards), and returns per launch
// and workgroup {start, marks 1-6, end} in s_memrealtime ticks (100 MHz).
extern "C" int mio_hip_llm_timeline(mio_hip_llm *m, uint64_t *out, int max_launches, int *n_launches) {
    MIO_REQUIRE(m && out && n_launches && m->graph, MIO_ERR_INVALID, "llm_timeline: run generate/eval first");
    int rc = mio::bind(m->d);
    if (rc) return rc;
    // the timeline replays the plain step (issue_step without the chain launch, which records no
    // marks), whatever the handle's sampling settings: the count leaves kind 14 out
    const int nl = (int)step_kinds(m).size() - (chain_on(m->sampling) ? 1 : 0);
    MIO_REQUIRE(max_launches >= nl, MIO_ERR_INVALID, "llm_timeline: need %d launch slots", nl);
    hipStream_t s = m->d->stream;
    const size_t nslot = (size_t)nl * mio::kTlSlots * 8;  // MIO_TL_SLOT: kTlSlots workgroup slots per launch
    mio::Scratch<unsigned long long> tl;
    MIO_HIP_CHECK(hipMalloc((void **)tl.put(), sizeof(unsigned long long) * nslot));
    mio::GraphExec ge;
    if ((rc = mio::capture_graph(s, [&] { return issue_step(m, tl); }, ge.put()))) return rc;
    for (int rep = 0; rep < 3; ++rep) {
        MIO_HIP_CHECK(hipMemsetAsync(tl, 0, sizeof(unsigned long long) * nslot, s));
        MIO_HIP_CHECK(hipGraphLaunch(ge, s));
    }
    std::vector<unsigned long long> h(nslot);
    MIO_HIP_CHECK(hipMemcpyAsync(h.data(), tl, sizeof(unsigned long long) * nslot, hipMemcpyDeviceToHost, s));
    MIO_HIP_CHECK(hipStreamSynchronize(s));
    std::memcpy(out, h.data(), sizeof(unsigned long long) * nslot);
    *n_launches = nl;
    return MIO_OK;
}
