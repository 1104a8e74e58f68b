// LLM decode runtime (see llm.h): one hipGraph per decode step, device-side sampling, C-ABI
// (include/mio_hip.h). The load is llm_load.cpp, the batched engine llm_batch.cpp, the
// parity-test entry points and diagnostics llm_diag.cpp; llm_model.h is what they share.
//
// Replaces, for the MioTTS path: the prefill llama_decode (test-to-speech.cpp:132-148), the
// decode loop llama_sampler_sample / llama_decode (:164-192) and the temp+dist sampler chain
// (:127-130).
#include <algorithm>
#include <cstring>

#include "llm_model.h"

// steps per replayed step graph (MIO_GRAPH_STEPS, 1..64; A/B knob, default 8)
int graph_steps() {
    static const int n = env_int("MIO_GRAPH_STEPS", 8, 1, 64);
    return n;
}

// MIO_NO_GRAPH=1: eager launches (rocprofv3 kernel tracing of graph replays crashes on
// ROCm 7.2 here; kernels and arguments are identical either way)
bool no_graph() {
    static const bool eager = env_flag("MIO_NO_GRAPH", false);
    return eager;
}

// MIO_ATT_FUSE_O (default 1): attention + O as one launch (k_att_o, kAttO) where the head
// shape has it; 0 keeps the two launches (A/B).
bool fuse_att_o(const mio_hip_llm *m) {
    static const bool env = env_flag("MIO_ATT_FUSE_O", true);
    return env && m->dims.n_kv <= mio::kRdyOff && mio::att_o_supported(m->dims.hd, m->dims.n_head / m->dims.n_kv);
}

// MIO_LAYER_ATT (default 1): layers >= 1 run their whole attention block as one launch
// (k_layer_att, kLayerAtt) where it is instantiated; 0 keeps attn_in + the k_att_o launch.
// MIO_LAYER_ATT: unset = measured policy, "0" = never, "1" = wherever instantiated. The policy
// leaves the hd 64 / 3-query-head shape (0.1B) on attn_in + k_att_o: its q|k|v hand-off inside
// the launch costs more than the boundary it removes (C2 93.0x fused vs 97.5x, and 86.8-89.1x
// vs 97.4x with 4 polls in flight; 1.7B Q4_K_M 54.27x vs 53.8x, 2.6B 35.43x vs 35.16x, 1.7B BF16
// even: profiles/r05_layer_att_policy.txt).
bool fuse_layer_att(const mio_hip_llm *m, int il) {
    static const int env = !env_flag("MIO_LAYER_ATT", true) ? 0 : (env_flag("MIO_LAYER_ATT", false) ? 1 : -1);
    if (env == 0 || il == 0 || !fuse_att_o(m) || !mio::layer_att_supported(m->dims, m->layers[il])) return false;
    const mio::LlmDims &d = m->dims;
    return env == 1 || !(d.hd == 64 && d.n_head == 3 * d.n_kv);
}

// MIO_FFN_FUSE (default 1): the FFN pair of a layer as one launch (k_ffn, kFfn) where it
// is instantiated (ffn_fused_supported); 0 keeps k_ffn_in + k_ffn_down (A/B).
// A Q8_0 gate|up beside a Q6_K down is fused where the file stores the gate|up as Q8_0 (the 0.1B
// Q6_K file: 0.396 vs 0.412 ms per step, profiles/q6k/fused_vs_separate.txt). The use_more_bits
// layers of a 0.1B Q4_K_M file reach the same pair of types with Q5_0 gate|up run as Q8_0: they
// keep the two launches they always had (never measured fused).
bool fuse_ffn(const mio_hip_llm *m, int il) {
    static const bool env = env_flag("MIO_FFN_FUSE", true);
    const mio::LayerW &L = m->layers[il];
    if (L.gate.type == 8 && L.down.type == 14 && m->gate_repacked[il]) return false;
    return env && mio::ffn_fused_supported(m->dims, L);
}

// Can this model run launch `kind` on layer il: the attention launches need an attention
// layer, the conv launches an lfm2 short-conv layer, a fused launch its switch and its
// instantiation. The unfused launches exist for every layer of their sort, whatever the step
// plan uses.
bool kind_in_layer(const mio_hip_llm *m, mio::StepKind kind, int il) {
    const bool conv = m->layers[il].conv != 0;
    switch (kind) {
        case mio::kAttnIn:
        case mio::kAttention:
        case mio::kAttnOut: return !conv;
        case mio::kConvIn:
        case mio::kConvOut: return conv;
        case mio::kAttO: return !conv && fuse_att_o(m);
        case mio::kLayerAtt: return !conv && fuse_layer_att(m, il);
        case mio::kFfn: return fuse_ffn(m, il);
        case mio::kFfnIn:
        case mio::kFfnDown:
        case mio::kLmHead:
        case mio::kSample: return true;
        default: return false;
    }
}

// Launches of layer il in step order: the most fused form kind_in_layer allows of the
// attention block (or the short conv's two launches), then of the FFN pair. Returns the count
// (<= kLayerKindsMax).
int layer_kinds(const mio_hip_llm *m, int il, mio::StepKind *w) {
    auto has = [&](mio::StepKind k) { return kind_in_layer(m, k, il); };
    int n = 0;
    if (has(mio::kConvIn))
        w[n++] = mio::kConvIn, w[n++] = mio::kConvOut;
    else if (has(mio::kLayerAtt))
        w[n++] = mio::kLayerAtt;
    else if (has(mio::kAttO))
        w[n++] = mio::kAttnIn, w[n++] = mio::kAttO;
    else
        w[n++] = mio::kAttnIn, w[n++] = mio::kAttention, w[n++] = mio::kAttnOut;
    if (has(mio::kFfn))
        w[n++] = mio::kFfn;
    else
        w[n++] = mio::kFfnIn, w[n++] = mio::kFfnDown;
    return n;
}

// A sampler-chain knob is off its neutral value: the step gains the chain launch.
bool chain_on(const mio::SamplingParams &sp) {
    return sp.top_k > 0 || sp.top_p < 1.0f || sp.min_p > 0.0f || sp.repeat_penalty != 1.0f ||
           sp.frequency_penalty != 0.0f || sp.presence_penalty != 0.0f;
}

int check_chain(const mio::SamplingParams &sp, const char *who) {
    const float f[5] = {sp.top_p, sp.min_p, sp.repeat_penalty, sp.frequency_penalty, sp.presence_penalty};
    for (float v : f) MIO_REQUIRE(v == v, MIO_ERR_INVALID, "%s: a sampling parameter is NaN", who);
    MIO_REQUIRE(sp.repeat_penalty > 0.0f, MIO_ERR_INVALID, "%s: repeat_penalty %g must be > 0", who,
                (double)sp.repeat_penalty);
    MIO_REQUIRE(sp.repeat_last_n >= 0 && sp.repeat_last_n <= mio::kChainHistMax, MIO_ERR_INVALID,
                "%s: repeat_last_n %d outside 0..%d", who, sp.repeat_last_n, mio::kChainHistMax);
    return MIO_OK;
}

// every launch of a step in order: the layers', then lm_head, then the sampler chain where the
// handle's sampling settings (mio_hip_llm_set_sampling) turn it on
std::vector<mio::StepKind> step_kinds(const mio_hip_llm *m) {
    std::vector<mio::StepKind> k;
    mio::StepKind w[kLayerKindsMax];
    for (int il = 0; il < m->n_layer; ++il) k.insert(k.end(), w, w + layer_kinds(m, il, w));
    k.push_back(mio::kLmHead);
    if (chain_on(m->sampling)) k.push_back(mio::kSampleChain);
    return k;
}

// One decode step on m->d->stream (tl: optional step timeline, diagnostic; chain: with the
// sampler chain launch behind lm_head).
int issue_step(mio_hip_llm *m, unsigned long long *tl, bool chain) {
    hipStream_t s = m->d->stream;
    int seq = 0;
    auto bufs = [&]() {
        mio::LlmBuffers b = m->buf;
        if (tl) b.tl = tl, b.seq = seq++;
        return b;
    };
    mio::StepKind w[kLayerKindsMax];
    for (int il = 0; il < m->n_layer; ++il)
        for (int i = 0, n = layer_kinds(m, il, w); i < n; ++i) mio::launch_step_kernel(w[i], m->ctx(), il, bufs(), s);
    mio::launch_step_kernel(mio::kLmHead, m->ctx(), 0, bufs(), s);
    if (chain) mio::launch_step_kernel(mio::kSampleChain, m->ctx(), 0, m->buf, s);
    return MIO_OK;
}

// The sampler of the last issued step (the step graph samples each token inside the next
// step's layer-0 attn_in): leaves the state with no pending sample.
int flush_sample(mio_hip_llm *m) {
    mio::launch_step_kernel(mio::kSample, m->ctx(), 0, m->buf, m->d->stream);
    MIO_HIP_CHECK(hipGetLastError());
    return MIO_OK;
}

// The step graphs: the plain pair always; chain: also the pair whose steps carry the sampler
// chain launch (captured on the first generate that needs it, beside the plain pair, so
// toggling the chain never re-captures either).
int ensure_graph(mio_hip_llm *m, bool chain) {
    auto steps = [m](int n, bool ch) {
        return [m, n, ch] {
            int rc = MIO_OK;
            for (int i = 0; i < n && !rc; ++i) rc = issue_step(m, nullptr, ch);
            return rc;
        };
    };
    int rc;
    if (!m->graph && (rc = mio::capture_graph(m->d->stream, steps(1, false), m->graph.put()))) return rc;
    if (!m->graph_n && (rc = mio::capture_graph(m->d->stream, steps(graph_steps(), false), m->graph_n.put())))
        return rc;
    if (!chain) return MIO_OK;
    if (!m->graph_c && (rc = mio::capture_graph(m->d->stream, steps(1, true), m->graph_c.put()))) return rc;
    if (!m->graph_cn && (rc = mio::capture_graph(m->d->stream, steps(graph_steps(), true), m->graph_cn.put())))
        return rc;
    return MIO_OK;
}

int put_cfg(mio_hip_llm *m, mio::SampleCfg c) {
    m->cfg = c;
    MIO_HIP_CHECK(hipMemcpyAsync(m->d_cfg, &c, sizeof(c), hipMemcpyHostToDevice, m->d->stream));
    return MIO_OK;
}

// Greedy over the whole vocabulary, no end token, next tokens forced from m->d_force where it
// says so (eval, eval_layers, the forced-step prefill).
mio::SampleCfg greedy_cfg(const mio_hip_llm *m) {
    mio::SampleCfg c{};
    c.temp = 0.0f, c.lo = 0, c.hi = m->dims.n_vocab, c.eos0 = c.eos1 = -1;
    c.force = m->d_force, c.n_force = m->max_steps, c.out_tokens = m->d_tokens, c.max_steps = m->max_steps;
    return c;
}

// A generate's sampler with sp's chain knobs (sp.seed is not read: a batch has one seed per stream): tokens to
// out_tokens, the end token's host word host_done (device address). force / n_force stay
// null / 0: the single-stream generate sets its own.
mio::SampleCfg sample_cfg(const mio_hip_llm *m, const mio::SamplingParams &sp, uint64_t seed, int *out_tokens,
                          int *host_done, int max_steps) {
    mio::SampleCfg c{};
    c.temp = sp.temperature;
    c.seed_lo = (uint32_t)seed, c.seed_hi = (uint32_t)(seed >> 32);
    c.lo = sp.allow_lo < 0 ? 0 : sp.allow_lo;
    c.hi = (sp.allow_hi < 0 || sp.allow_hi > m->dims.n_vocab) ? m->dims.n_vocab : sp.allow_hi;
    c.eos0 = sp.eos0, c.eos1 = sp.eos1;
    c.force = nullptr, c.n_force = 0;
    c.out_tokens = out_tokens, c.max_steps = max_steps;
    c.host_done = host_done;
    c.top_k = sp.top_k, c.top_p = sp.top_p, c.min_p = sp.min_p;
    c.repeat_penalty = sp.repeat_penalty, c.frequency_penalty = sp.frequency_penalty;
    c.presence_penalty = sp.presence_penalty, c.repeat_last_n = sp.repeat_last_n;
    c.first_step = 0;  // the caller's: the first step whose token is sampled
    return c;
}

int set_state(mio_hip_llm *m, int pos, int token, int step) {
    if (int rc = reset_tickets(m)) return rc;
    mio::StepState st{pos, step, token, 0};
    MIO_HIP_CHECK(hipMemcpyAsync(m->buf.st, &st, sizeof(st), hipMemcpyHostToDevice, m->d->stream));
    mio::launch_embed_token(m->dims, m->tok, m->buf, m->d->stream);
    MIO_HIP_CHECK(hipGetLastError());
    return MIO_OK;
}

// The attention chunk tickets (attn_merge_last) are zeroed in stream order before every
// prefill, every decode start and every batched generate (the last chunk workgroup of each
// attention launch resets its ticket, so they are 0 here anyway; this keeps an interrupted
// run from carrying a count).
int reset_tickets(mio_hip_llm *m) {
    MIO_HIP_CHECK(hipMemsetAsync(m->buf.att_cnt, 0, (size_t)mio::kAttCntInts * sizeof(int), m->d->stream));
    MIO_HIP_CHECK(hipMemsetAsync(m->pf.att_cnt, 0, (size_t)mio::kPrefillB * m->dims.n_kv * sizeof(int), m->d->stream));
    MIO_HIP_CHECK(hipMemsetAsync(m->pf.qcnt, 0, (size_t)mio::kQcntInts * sizeof(int), m->d->stream));
    return MIO_OK;
}

// The fused launches' hand-off counters (att_cnt from kRdyOff on) are zeroed by the launch
// after them in a step; a diagnostic that runs one alone zeroes them itself.
int reset_rdy(mio_hip_llm *m, hipStream_t s) {
    MIO_HIP_CHECK(hipMemsetAsync(m->buf.att_cnt + mio::kRdyOff, 0,
                                 (size_t)(mio::kAttCntInts - mio::kRdyOff) * sizeof(int), s));
    return MIO_OK;
}

// k_att_o's bounded wait (wait_count) raises att_cnt[kRdyFlag] if a merge signal never came:
// reported as an error instead of silently using stale attention outputs.
int check_handoff(mio_hip_llm *m) {
    bool any = fuse_att_o(m);
    for (int il = 0; il < m->n_layer && !any; ++il) any = fuse_ffn(m, il);
    if (!any) return MIO_OK;
    int flag = 0;
    int *f = m->buf.att_cnt + mio::kRdyFlag;
    MIO_HIP_CHECK(hipMemcpyAsync(&flag, f, sizeof(int), hipMemcpyDeviceToHost, m->d->stream));
    MIO_HIP_CHECK(hipStreamSynchronize(m->d->stream));
    if (flag) {
        MIO_HIP_CHECK(hipMemsetAsync(f, 0, sizeof(int), m->d->stream));
        mio::set_error("llm decode: an in-launch hand-off wait (attention -> O, or gate|up -> down) timed out");
        return MIO_ERR_HIP;
    }
    return MIO_OK;
}

namespace {

// Batched prefill of prompt positions [0, n) (tokens already in m->d_prompt): chunks of
// kPrefillB tokens, one weight pass per launch (llm_prefill.hip). MIO_SEQ_PREFILL=1 is not
// handled here (see llm_begin).
int prefill_issue(mio_hip_llm *m, int n) {
    for (int p0 = 0; p0 < n; p0 += mio::kPrefillB) {
        const int nt = n - p0 < mio::kPrefillB ? n - p0 : mio::kPrefillB;
        mio::PrefillBuffers pb = m->pf;
        pb.pos = m->d_iota + p0, pb.pos_stride = 1;  // positions p0 .. p0 + nt - 1
        pb.seq = m->d_iota, pb.seq_stride = 0;       // one sequence: the model's own cache
        pb.seq_kv = 0;
        mio::launch_prefill_chunk(m->dims, m->layers.data(), m->n_layer, m->kc, m->vc, m->tok, pb, p0, nt,
                                  (p0 + nt - 1) / mio::kAttChunk + 1, m->d->stream);
        MIO_HIP_CHECK(hipGetLastError());
    }
    return MIO_OK;
}

int upload_prompt(mio_hip_llm *m, const int32_t *prompt, int n) {
    if (int rc = reset_tickets(m)) return rc;
    MIO_HIP_CHECK(hipMemcpyAsync(m->d_prompt, prompt, (size_t)n * 4, hipMemcpyHostToDevice, m->d->stream));
    return MIO_OK;
}

bool sequential_prefill() {
    static const bool seq = env_flag("MIO_SEQ_PREFILL", false);
    return seq;
}

// weight passes over P prompt positions: one per chunk of the batched prefill, one per position
// as forced decode steps (MIO_SEQ_PREFILL=1, or a model the multi-token engine does not take)
int prompt_passes(const mio_hip_llm *m, int P) {
    return sequential_prefill() || !m->bf16_mt() ? P : (P + mio::kPrefillB - 1) / mio::kPrefillB;
}

// force[j] = the token step j's sampler is forced to: tokens[j + 1] for the prompt, -1 after it
int upload_force(mio_hip_llm *m, const int32_t *tokens, int n) {
    std::vector<int> force(m->max_steps, -1);
    for (int j = 0; j + 1 < n && j < m->max_steps; ++j) force[j] = tokens[j + 1];
    MIO_HIP_CHECK(hipMemcpyAsync(m->d_force, force.data(), force.size() * 4, hipMemcpyHostToDevice, m->d->stream));
    return MIO_OK;
}

// Drops every outstanding snapshot (waits for its copies: the host buffers are reused).
int snaps_drain(mio_hip_llm *m) {
    for (; m->snap_n > 0; --m->snap_n, m->snap_head = (m->snap_head + 1) % mio_hip_llm::kSnaps)
        MIO_HIP_CHECK(hipEventSynchronize(m->snaps[m->snap_head].ev));
    return MIO_OK;
}

// Enqueues a snapshot of the state and of the token ring slots the issued steps write.
int snap_push(mio_hip_llm *m) {
    if (m->snap_n == mio_hip_llm::kSnaps) {  // reuse the oldest slot: its copies must be done
        MIO_HIP_CHECK(hipEventSynchronize(m->snaps[m->snap_head].ev));
        m->snap_head = (m->snap_head + 1) % mio_hip_llm::kSnaps;
        --m->snap_n;
    }
    mio_hip_llm::Snap &sn = m->snaps[(m->snap_head + m->snap_n) % mio_hip_llm::kSnaps];
    const int first = m->n_prompt - 1;
    sn.hi = std::min(m->steps_issued, m->max_steps);
    sn.issued = m->steps_issued;
    MIO_HIP_CHECK(hipMemcpyAsync(sn.st, m->buf.st, sizeof(mio::StepState), hipMemcpyDeviceToHost, m->d->stream));
    if (sn.hi > first)
        MIO_HIP_CHECK(hipMemcpyAsync(sn.tok + first, m->d_tokens + first, (size_t)(sn.hi - first) * 4,
                                     hipMemcpyDeviceToHost, m->d->stream));
    MIO_HIP_CHECK(hipEventRecord(sn.ev, m->d->stream));
    ++m->snap_n;
    return MIO_OK;
}

// n decode steps: eagerly under MIO_NO_GRAPH, or as graph_steps()-step graphs and 1-step ones
int run_steps(mio_hip_llm *m, int n) {
    if (no_graph()) {
        for (int i = 0; i < n; ++i)
            if (int rc = issue_step(m, nullptr, m->chain)) return rc;
        return MIO_OK;
    }
    hipGraphExec_t g1 = m->chain ? m->graph_c : m->graph, gn = m->chain ? m->graph_cn : m->graph_n;
    for (const int gs = graph_steps(); n >= gs; n -= gs) MIO_HIP_CHECK(hipGraphLaunch(gn, m->d->stream));
    for (; n > 0; --n) MIO_HIP_CHECK(hipGraphLaunch(g1, m->d->stream));
    return MIO_OK;
}

}  // namespace

// Batched prefill of positions [0, n): every launch reads only device buffers whose addresses
// depend on n alone (prompt tokens in m->d_prompt), so one graph per prompt length replays it.
// The first prefill of a length runs eagerly (its launches set the kernels' LDS attributes
// outside any capture), the second too and is captured, later ones replay the graph.
// MIO_PREFILL_GRAPH=0 or MIO_NO_GRAPH=1 (every launch eager, for kernel tracing): eager.
int prefill(mio_hip_llm *m, int n) {
    static const bool use_graph = env_flag("MIO_PREFILL_GRAPH", true) && !no_graph();
    if (n <= 0) return MIO_OK;
    const auto it = m->prefill_graphs.find(n);
    if (use_graph && it != m->prefill_graphs.end()) {
        MIO_HIP_CHECK(hipGraphLaunch(it->second, m->d->stream));
        return MIO_OK;
    }
    int rc = prefill_issue(m, n);
    // a length is captured when it comes back (the second prefill of that length): a one-off
    // prompt does not pay for a capture it never replays
    if (rc || !use_graph || m->prefill_graphs.size() >= 16 || m->prefill_seen[n]++ == 0) return rc;
    // capture a second issue for the next utterance of this length; the prefill above already
    // ran eagerly, so a failed capture or instantiation only leaves this length uncached
    mio::GraphExec ge;
    if (mio::capture_graph(m->d->stream, [&] { return prefill_issue(m, n); }, ge.put()) == MIO_OK)
        m->prefill_graphs[n] = std::move(ge);
    (void)hipGetLastError();
    return MIO_OK;
}

int run_wait(mio_hip_llm *m, int k) {
    if (k >= kRunDepth) MIO_HIP_CHECK(hipEventSynchronize(m->run_ev[k - kRunDepth]));
    return MIO_OK;
}

int run_mark(mio_hip_llm *m, int k) {
    if ((int)m->run_ev.size() <= k) {
        m->run_ev.emplace_back();
        MIO_HIP_CHECK(hipEventCreate(m->run_ev.back().put()));
    }
    MIO_HIP_CHECK(hipEventRecord(m->run_ev[k], m->d->stream));
    return MIO_OK;
}

namespace mio {

LlmInfo llm_info(const mio_hip_llm *m) {
    return LlmInfo{m->dims.n_vocab, m->dims.n_embd, m->n_layer, m->dims.n_head, m->dims.n_kv,
                   m->dims.hd, m->dims.n_ff, m->dims.n_ctx};
}

uint64_t llm_step_weight_bytes(const mio_hip_llm *m) { return m->weight_bytes; }

int llm_begin(mio_hip_llm *m, const int32_t *prompt, int n_prompt, int max_new, const SamplingParams &sp) {
    MIO_REQUIRE(m && prompt && n_prompt >= 1 && max_new >= 1, MIO_ERR_INVALID, "llm_begin: bad args");
    MIO_REQUIRE(n_prompt <= m->dims.n_ctx, MIO_ERR_INVALID, "llm_begin: %d prompt tokens exceed n_ctx %d",
                n_prompt, m->dims.n_ctx);
    // the reference decodes until llama_decode fails at a full context and keeps the token
    // sampled last (test-to-speech.cpp:163-187): at most n_ctx - n_prompt + 1 new tokens
    max_new = std::min(max_new, m->dims.n_ctx - n_prompt + 1);
    for (int i = 0; i < n_prompt; ++i)
        MIO_REQUIRE(prompt[i] >= 0 && prompt[i] < m->dims.n_vocab, MIO_ERR_INVALID,
                    "llm_begin: token %d out of vocab", prompt[i]);
    int rc = check_chain(sp, "llm_begin");
    if (rc || (rc = mio::bind(m->d)) || (rc = snaps_drain(m)) || (rc = upload_force(m, prompt, n_prompt))) return rc;
    __atomic_store_n(m->host_done.get(), 0, __ATOMIC_SEQ_CST);  // the cfg copy below is stream-ordered behind it
    SampleCfg c = sample_cfg(m, sp, sp.seed, m->d_tokens, m->host_done_dev, m->max_steps);
    c.force = m->d_force, c.n_force = m->max_steps;
    c.first_step = n_prompt - 1;  // the prompt's forced steps are no history
    m->chain = chain_on(sp);
    if ((rc = put_cfg(m, c)) || (rc = ensure_graph(m, m->chain))) return rc;
    m->n_prompt = n_prompt;
    m->max_new = max_new;
    m->steps_total = n_prompt - 1 + max_new;
    // prompt positions [0, P) are prefilled here: batched (one weight pass per chunk of
    // kPrefillB tokens), or, with MIO_SEQ_PREFILL=1, as P forced decode steps; decoding
    // then starts at position P with the step counter at P either way (same sampler stream)
    const int P = n_prompt - 1;
    m->prompt_chunks = prompt_passes(m, P);
    if (sequential_prefill() || !m->bf16_mt()) {
        m->steps_issued = 0;
        if ((rc = set_state(m, 0, prompt[0]))) return rc;
        return llm_run(m, P);
    }
    if ((rc = upload_prompt(m, prompt, n_prompt)) || (rc = prefill(m, P))) return rc;
    m->steps_issued = P;
    return set_state(m, P, prompt[P], P);
}

int llm_run(mio_hip_llm *m, int n_steps) {
    int rc = mio::bind(m->d);
    if (rc) return rc;
    const int n = std::max(0, std::min(n_steps, m->steps_total - m->steps_issued));
    m->steps_issued += n;
    if ((rc = run_steps(m, n)) || (rc = flush_sample(m))) return rc;
    return snap_push(m);
}

int llm_graph_steps() { return graph_steps(); }

// Steps until the end: graphs of graph_steps() steps, at most kRunDepth queued ahead of the GPU
// (the host waits for the event of the graph kRunDepth back, while the next one still runs),
// and none issued once the sampler has stored the end token's host word. After an end token the
// rest of its graph and at most kRunDepth - 1 more run (returning at entry), instead of the
// rest of a 32-step poll interval and one more interval. Then the flush sampler + a snapshot
// (llm_poll collects the tokens).
int llm_run_to_end(mio_hip_llm *m) {
    int rc = mio::bind(m->d);
    if (rc) return rc;
    m->run_base = m->steps_issued;
    int k = 0;
    for (; m->steps_issued < m->steps_total; ++k) {
        if ((rc = run_wait(m, k))) return rc;
        if (__atomic_load_n(m->host_done.get(), __ATOMIC_ACQUIRE)) break;
        const int n = std::min(graph_steps(), m->steps_total - m->steps_issued);
        if ((rc = run_steps(m, n))) return rc;
        m->steps_issued += n;
        if ((rc = run_mark(m, k))) return rc;
    }
    m->run_graphs = k;
    if ((rc = flush_sample(m))) return rc;
    return snap_push(m);
}

int llm_poll(mio_hip_llm *m, std::vector<int32_t> &out, bool *done) {
    int rc = mio::bind(m->d);
    if (rc) return rc;
    if (m->snap_n == 0 && (rc = snap_push(m))) return rc;
    // the oldest outstanding snapshot: steps enqueued after it keep the GPU busy meanwhile
    const int slot = m->snap_head;
    const mio_hip_llm::Snap &sn = m->snaps[slot];
    MIO_HIP_CHECK(hipEventSynchronize(sn.ev));
    m->snap_head = (m->snap_head + 1) % mio_hip_llm::kSnaps;
    --m->snap_n;
    const int first = m->n_prompt - 1;
    const StepState st = *sn.st.get();
    const int n = std::min(st.step, sn.hi) > first ? std::min(st.step, sn.hi) - first : 0;
    out.assign(sn.tok + first, sn.tok + first + n);
    bool d = false;
    for (int i = 0; i < n; ++i)
        if (out[i] == m->cfg.eos0 || out[i] == m->cfg.eos1) {
            out.resize(i);  // the reference stops before appending the end token (:168-170)
            d = true;
            m->eos_snap = slot;
            break;
        }
    if (done) *done = d || sn.issued >= m->steps_total;
    return MIO_OK;
}

}  // namespace mio

extern "C" int mio_hip_llm_set_sampling(mio_hip_llm *m, const mio_sampling *s) {
    MIO_REQUIRE(m, MIO_ERR_INVALID, "llm_set_sampling: null handle");
    mio::SamplingParams sp;  // neutral
    if (s) {
        sp.top_k = s->top_k, sp.top_p = s->top_p, sp.min_p = s->min_p, sp.repeat_penalty = s->repeat_penalty;
        sp.frequency_penalty = s->frequency_penalty, sp.presence_penalty = s->presence_penalty;
        sp.repeat_last_n = s->repeat_last_n;
    }
    if (int rc = check_chain(sp, "llm_set_sampling")) return rc;
    m->sampling = sp;
    return MIO_OK;
}

extern "C" int mio_hip_llm_get_sampling(const mio_hip_llm *m, mio_sampling *s) {
    MIO_REQUIRE(m && s, MIO_ERR_INVALID, "llm_get_sampling: null");
    const mio::SamplingParams &sp = m->sampling;
    *s = mio_sampling{sp.top_k, sp.top_p, sp.min_p, sp.repeat_penalty, sp.frequency_penalty, sp.presence_penalty,
                      sp.repeat_last_n};
    return MIO_OK;
}

extern "C" int mio_hip_llm_load_ms(const mio_hip_llm *m, double *ms) {
    MIO_REQUIRE(m && ms, MIO_ERR_INVALID, "llm_load_ms: null");
    *ms = m->load_ms;
    return MIO_OK;
}

extern "C" int mio_hip_llm_prompt_chunks(const mio_hip_llm *m, int *chunks) {
    MIO_REQUIRE(m && chunks, MIO_ERR_INVALID, "llm_prompt_chunks: null");
    *chunks = m->prompt_chunks;
    return MIO_OK;
}

extern "C" int mio_hip_llm_graph_steps(void) { return graph_steps(); }

extern "C" int mio_hip_llm_steps_issued(const mio_hip_llm *m, int *steps) {
    MIO_REQUIRE(m && steps, MIO_ERR_INVALID, "llm_steps_issued: null");
    *steps = std::max(0, m->steps_issued - (m->n_prompt - 1));
    return MIO_OK;
}

extern "C" int mio_hip_llm_info(const mio_hip_llm *m, int *info) {
    MIO_REQUIRE(m && info, MIO_ERR_INVALID, "llm_info: null");
    mio::LlmInfo i = mio::llm_info(m);
    info[0] = i.n_vocab, info[1] = i.n_embd, info[2] = i.n_layer, info[3] = i.n_head;
    info[4] = i.n_kv, info[5] = i.head_dim, info[6] = i.n_ff, info[7] = i.n_ctx;
    return MIO_OK;
}

extern "C" int mio_hip_llm_weight_bytes(const mio_hip_llm *m, uint64_t *bytes) {
    MIO_REQUIRE(m && bytes, MIO_ERR_INVALID, "llm_weight_bytes: null");
    *bytes = m->weight_bytes;
    return MIO_OK;
}

extern "C" int mio_hip_llm_tail(const mio_hip_llm *m, int *steps, int *timed_steps, float *timed_ms) {
    MIO_REQUIRE(m && steps && timed_steps && timed_ms, MIO_ERR_INVALID, "llm_tail: null argument");
    *steps = m->tail_steps, *timed_steps = m->tail_timed_steps, *timed_ms = m->tail_ms;
    return MIO_OK;
}

extern "C" int mio_hip_llm_eval(mio_hip_llm *m, int32_t token, int pos, float *logits) {
    MIO_REQUIRE(m && token >= 0 && token < m->dims.n_vocab && pos >= 0 && pos < m->dims.n_ctx,
                MIO_ERR_INVALID, "llm_eval: bad token/pos");
    int rc = mio::bind(m->d);
    if (rc) return rc;
    if ((rc = put_cfg(m, greedy_cfg(m))) || (rc = ensure_graph(m))) return rc;
    const int zero = 0;
    MIO_HIP_CHECK(hipMemcpyAsync(m->d_force, &zero, 4, hipMemcpyHostToDevice, m->d->stream));
    if ((rc = set_state(m, pos, token))) return rc;
    MIO_HIP_CHECK(hipGraphLaunch(m->graph, m->d->stream));
    if (logits)
        MIO_HIP_CHECK(hipMemcpyAsync(logits, m->buf.logits, (size_t)m->dims.n_vocab * 4, hipMemcpyDeviceToHost,
                                     m->d->stream));
    // the step left its sample pending (k_lm_head): take it, so the state is a settled one
    if ((rc = flush_sample(m))) return rc;
    MIO_HIP_CHECK(hipStreamSynchronize(m->d->stream));
    return check_handoff(m);
}

extern "C" int mio_hip_llm_prefill(mio_hip_llm *m, const int32_t *tokens, int n_tokens, float *logits) {
    MIO_REQUIRE(m && tokens && n_tokens >= 1 && n_tokens <= m->dims.n_ctx, MIO_ERR_INVALID,
                "llm_prefill: bad args");
    for (int i = 0; i < n_tokens; ++i)
        MIO_REQUIRE(tokens[i] >= 0 && tokens[i] < m->dims.n_vocab, MIO_ERR_INVALID, "llm_prefill: token %d",
                    tokens[i]);
    int rc = mio::bind(m->d);
    if (rc) return rc;
    if (!m->bf16_mt()) {
        // forced decode steps as llm_begin runs them (BF16 beside int8 matrices is not on the
        // multi-token engine): step j decodes tokens[j] at position j and its sampler is forced
        // to tokens[j + 1]
        m->prompt_chunks = n_tokens - 1;
        if (n_tokens > 1) {
            if ((rc = upload_force(m, tokens, n_tokens)) || (rc = put_cfg(m, greedy_cfg(m))) ||
                (rc = ensure_graph(m)) || (rc = set_state(m, 0, tokens[0])))
                return rc;
            for (int j = 0; j + 1 < n_tokens; ++j) MIO_HIP_CHECK(hipGraphLaunch(m->graph, m->d->stream));
        }
    } else {
        m->prompt_chunks = (n_tokens - 1 + mio::kPrefillB - 1) / mio::kPrefillB;
        if ((rc = upload_prompt(m, tokens, n_tokens)) || (rc = prefill(m, n_tokens - 1))) return rc;
    }
    return mio_hip_llm_eval(m, tokens[n_tokens - 1], n_tokens - 1, logits);
}

extern "C" int mio_hip_llm_logits(mio_hip_llm *m, float *logits) {
    MIO_REQUIRE(m && logits, MIO_ERR_INVALID, "llm_logits: null");
    int rc = mio::bind(m->d);
    if (rc) return rc;
    MIO_HIP_CHECK(hipMemcpyAsync(logits, m->buf.logits, (size_t)m->dims.n_vocab * 4, hipMemcpyDeviceToHost,
                                 m->d->stream));
    MIO_HIP_CHECK(hipStreamSynchronize(m->d->stream));
    return MIO_OK;
}

extern "C" int mio_hip_llm_generate(mio_hip_llm *m, const int32_t *prompt, int n_prompt, int max_tokens,
                                    float temperature, uint64_t seed, int32_t allow_lo, int32_t allow_hi,
                                    int32_t eos0, int32_t eos1, int32_t check_interval, int32_t *out_tokens,
                                    int *n_out) {
    MIO_REQUIRE(m && out_tokens && n_out, MIO_ERR_INVALID, "llm_generate: null argument");
    mio::SamplingParams sp = m->sampling;  // the chain knobs (mio_hip_llm_set_sampling)
    sp.temperature = temperature, sp.seed = seed, sp.allow_lo = allow_lo, sp.allow_hi = allow_hi;
    sp.eos0 = eos0, sp.eos1 = eos1;
    int rc = mio::llm_begin(m, prompt, n_prompt, max_tokens, sp);
    if (rc) return rc;
    (void)check_interval;  // the end token reaches the host through its mapped word (r06)
    std::vector<int32_t> toks;
    bool done = false;
    m->eos_snap = -1, m->tail_steps = 0, m->tail_timed_steps = 0, m->tail_ms = 0.0f;
    if ((rc = mio::llm_run_to_end(m))) return rc;
    if ((rc = mio::llm_poll(m, toks, &done))) return rc;
    if (m->eos_snap >= 0) {
        // steps after the end token's: they return at entry (StepState.done). The end token is
        // sampled by step e + 1 (inside its layer-0 launch, or the flush after the last graph);
        // the graphs queued after the one holding that step are timed by their events
        const int e1 = (n_prompt - 1) + (int)toks.size() + 1;
        m->tail_steps = m->steps_issued - e1;
        const int gs = mio::llm_graph_steps();
        const int g = (e1 - 1 - m->run_base) / gs;  // step numbers are 0-based: e1 - 1 is step e + 1
        if (g >= 0 && g + 1 < m->run_graphs) {
            MIO_HIP_CHECK(hipEventSynchronize(m->run_ev[m->run_graphs - 1]));
            MIO_HIP_CHECK(hipEventElapsedTime(&m->tail_ms, m->run_ev[g], m->run_ev[m->run_graphs - 1]));
            m->tail_timed_steps = m->steps_issued - std::min(m->steps_total, m->run_base + (g + 1) * gs);
        }
    }
    if ((rc = check_handoff(m))) return rc;
    const int n = (int)toks.size() < max_tokens ? (int)toks.size() : max_tokens;
    std::memcpy(out_tokens, toks.data(), (size_t)n * 4);
    *n_out = n;
    return MIO_OK;
}
