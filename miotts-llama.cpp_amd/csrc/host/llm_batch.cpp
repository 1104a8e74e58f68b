// Batched decode engine of the LLM runner (see llm.h, llm_model.h): B independent utterances
// decoded together on the multi-token layers (csrc/hip/llm_prefill.hip), one weight pass per
// step for all of them.
#include <algorithm>
#include <cstring>
#include <vector>

#include "llm_model.h"

namespace {

size_t batch_seq_ring(const mio_hip_llm *m) { return (size_t)m->n_layer * mio::kConvSlots * m->dims.n_embd; }

// Batch state for B streams (re-allocated when B changes; graphs re-captured).
int batch_ensure(mio_hip_llm *m, int B) {
    auto &bt = m->bt;
    if (bt.B == B) return MIO_OK;
    bt.graph.reset(), bt.graph_n.reset(), bt.graph_c.reset(), bt.graph_cn.reset();
    for (void *p : bt.allocs) hipFree(p);
    bt.allocs.clear();
    bt.B = 0;
    const mio::LlmDims &D = m->dims;
    const size_t seq_kv = (size_t)m->n_layer * D.n_kv * D.n_ctx * D.hd;
    auto al = [&](size_t bytes) -> void * {
        void *p = nullptr;
        if (hipMalloc(&p, bytes + 256) != hipSuccess) return nullptr;
        bt.allocs.push_back(p);
        // stream-ordered: the runner's stream is non-blocking, so a null-stream memset could
        // still be clearing the caches while the prefill below writes them
        hipMemsetAsync(p, 0, bytes + 256, m->d->stream);
        return p;
    };
    bt.kc = (_Float16 *)al((size_t)B * seq_kv * 2);
    bt.vc = (_Float16 *)al((size_t)B * seq_kv * 2);
    bt.st = (mio::StepState *)al((size_t)B * sizeof(mio::StepState));
    bt.cfg = (mio::SampleCfg *)al((size_t)B * sizeof(mio::SampleCfg));
    bt.logits = (float *)al((size_t)B * D.n_vocab * 4);
    bt.smp = (float *)al((size_t)B * mio::lm_head_blocks(D) * 2 * 4);
    bt.tokens = (int *)al((size_t)B * D.n_ctx * 4);
    bt.ppos = (int *)al((size_t)B * D.n_ctx * 4);
    bt.pseq = (int *)al((size_t)B * D.n_ctx * 4);
    bt.ptok = (int *)al((size_t)B * D.n_ctx * 4);
    bt.ring = m->buf.ring ? (float *)al(B * batch_seq_ring(m) * 4) : nullptr;
    if (!bt.kc || !bt.vc || !bt.st || !bt.cfg || !bt.logits || !bt.smp || !bt.tokens || !bt.ppos || !bt.pseq ||
        !bt.ptok || (m->buf.ring && !bt.ring)) {
        for (void *p : bt.allocs) hipFree(p);
        bt.allocs.clear();
        mio::set_error("llm_generate_batch: device allocation for %d streams failed", B);
        return MIO_ERR_OOM;
    }
    bt.B = B;
    MIO_HIP_CHECK(hipStreamSynchronize(m->d->stream));
    return MIO_OK;
}

// The multi-token layers' view of the batch: token t sits at position pos[t * pos_stride] of
// stream seq[t] (its cache and short-conv ring).
mio::PrefillBuffers batch_pb(mio_hip_llm *m, const int *pos, int pos_stride, const int *seq) {
    mio::PrefillBuffers pb = m->pf;
    pb.pos = pos, pb.pos_stride = pos_stride;
    pb.seq = seq, pb.seq_stride = 1;
    pb.seq_kv = (size_t)m->n_layer * m->dims.n_kv * m->dims.n_ctx * m->dims.hd;
    pb.ring = m->bt.ring, pb.seq_ring = batch_seq_ring(m);
    return pb;
}

// the decode step's view: stream b's position is st[b].pos, its cache is b
mio::PrefillBuffers step_pb(mio_hip_llm *m) {
    return batch_pb(m, &m->bt.st[0].pos, (int)(sizeof(mio::StepState) / sizeof(int)), m->d_iota);
}

mio::BatchBuffers batch_bb(mio_hip_llm *m) { return mio::BatchBuffers{m->bt.st, m->bt.cfg, m->bt.logits, m->bt.smp}; }

int issue_batch_steps(mio_hip_llm *m, int n, bool chain) {
    for (int i = 0; i < n; ++i)
        mio::launch_batch_step(m->dims, m->layers.data(), m->n_layer, m->bt.kc, m->bt.vc, m->out_norm, m->lm, m->tok,
                               step_pb(m), batch_bb(m), m->bt.B, chain, m->d->stream);
    return MIO_OK;
}

// n batched steps: the first ever step for this B runs eagerly (its launches set the
// kernels' LDS attributes outside any capture), then 1- and graph_steps()-step graphs replay.
// chain: the steps carry the sampler chain launch; they have a graph pair of their own.
int run_batch(mio_hip_llm *m, int n, bool chain) {
    auto &bt = m->bt;
    hipStream_t s = m->d->stream;
    mio::GraphExec &g1 = chain ? bt.graph_c : bt.graph, &gn = chain ? bt.graph_cn : bt.graph_n;
    if (n > 0 && (no_graph() || !g1)) {
        issue_batch_steps(m, no_graph() ? n : 1, chain);
        MIO_HIP_CHECK(hipGetLastError());
        if (no_graph()) return MIO_OK;
        --n;
        int rc;
        if ((rc = mio::capture_graph(s, [m, chain] { return issue_batch_steps(m, 1, chain); }, g1.put())) ||
            (rc = mio::capture_graph(s, [m, chain] { return issue_batch_steps(m, graph_steps(), chain); }, gn.put())))
            return rc;
    }
    for (const int gs = graph_steps(); n >= gs; n -= gs) MIO_HIP_CHECK(hipGraphLaunch(gn, s));
    for (; n > 0; --n) MIO_HIP_CHECK(hipGraphLaunch(g1, s));
    return MIO_OK;
}

}  // namespace

// B independent utterances decoded together (the reference runs them one after another, one
// llama_context each: test-to-speech.cpp:94-199 per call). Prompts are concatenated;
// stream b's sampled tokens go to out_tokens[b * max_tokens ...], n_out[b] of them (up to,
// not including, an end token). Each stream's tokens equal a single-stream generate with
// its seed (same kernels' arithmetic per token, same sampler noise).
extern "C" int mio_hip_llm_generate_batch(mio_hip_llm *m, const int32_t *prompts, const int32_t *prompt_lens, int B,
                                          int max_tokens, float temperature, const uint64_t *seeds,
                                          int32_t allow_lo, int32_t allow_hi, int32_t eos0, int32_t eos1,
                                          int32_t check_interval, int32_t *out_tokens, int32_t *n_out) {
    MIO_REQUIRE(m && prompts && prompt_lens && seeds && out_tokens && n_out && max_tokens >= 1, MIO_ERR_INVALID,
                "llm_generate_batch: bad args");
    MIO_REQUIRE(mio::batch_supported(m->dims, B, m->lm.type), MIO_ERR_UNSUPPORTED,
                "llm_generate_batch: %d streams not supported (1..%d, lm_head LDS)", B, mio::kBatchMax);
    MIO_REQUIRE(m->bf16_mt(), MIO_ERR_UNSUPPORTED,
                "llm_generate_batch: BF16 weights mixed with quantized ones run on the single-stream decode "
                "only (mio_hip_llm_generate)");
    const mio::LlmDims &D = m->dims;
    std::vector<int> off(B + 1, 0);
    for (int b = 0; b < B; ++b) {
        MIO_REQUIRE(prompt_lens[b] >= 1 && prompt_lens[b] <= D.n_ctx, MIO_ERR_INVALID,
                    "llm_generate_batch: stream %d: %d prompt tokens exceed n_ctx %d", b, prompt_lens[b], D.n_ctx);
        off[b + 1] = off[b] + prompt_lens[b];
    }
    for (int i = 0; i < off[B]; ++i)
        MIO_REQUIRE(prompts[i] >= 0 && prompts[i] < D.n_vocab, MIO_ERR_INVALID,
                    "llm_generate_batch: token %d out of vocab", prompts[i]);
    int rc = mio::bind(m->d);
    if (rc || (rc = batch_ensure(m, B)) || (rc = reset_tickets(m))) return rc;
    auto &bt = m->bt;
    hipStream_t s = m->d->stream;
    // prompt positions [0, P_b) of every stream: one flattened list, kPrefillB tokens per
    // chunk whatever stream they belong to (one weight pass per chunk)
    std::vector<int> ftok, fpos, fseq;
    for (int b = 0; b < B; ++b)
        for (int p = 0; p + 1 < prompt_lens[b]; ++p) {
            ftok.push_back(prompts[off[b] + p]);
            fpos.push_back(p);
            fseq.push_back(b);
        }
    const int nf = (int)ftok.size();
    if (nf) {
        MIO_HIP_CHECK(hipMemcpyAsync(bt.ptok, ftok.data(), (size_t)nf * 4, hipMemcpyHostToDevice, s));
        MIO_HIP_CHECK(hipMemcpyAsync(bt.ppos, fpos.data(), (size_t)nf * 4, hipMemcpyHostToDevice, s));
        MIO_HIP_CHECK(hipMemcpyAsync(bt.pseq, fseq.data(), (size_t)nf * 4, hipMemcpyHostToDevice, s));
    }
    for (int c0 = 0; c0 < nf; c0 += mio::kPrefillB) {
        const int nt = nf - c0 < mio::kPrefillB ? nf - c0 : mio::kPrefillB;
        int pmax = 0;
        for (int t = 0; t < nt; ++t) pmax = std::max(pmax, fpos[c0 + t]);
        mio::PrefillBuffers pb = batch_pb(m, bt.ppos + c0, 1, bt.pseq + c0);
        pb.tokens = bt.ptok;
        mio::launch_prefill_chunk(D, m->layers.data(), m->n_layer, bt.kc, bt.vc, m->tok, pb, c0, nt,
                                  pmax / mio::kAttChunk + 1, s);
        MIO_HIP_CHECK(hipGetLastError());
    }
    // per-stream state: decoding starts at position P_b = len_b - 1 with the step counter at
    // P_b (the single-stream generate's sampler stream)
    mio::SamplingParams sp = m->sampling;  // the chain knobs, shared by every stream
    sp.temperature = temperature, sp.allow_lo = allow_lo, sp.allow_hi = allow_hi, sp.eos0 = eos0, sp.eos1 = eos1;
    const bool chain = chain_on(sp);
    std::vector<mio::StepState> st(B);
    std::vector<mio::SampleCfg> cf(B);
    std::vector<int> budget(B);
    for (int b = 0; b < B; ++b) {
        const int P = prompt_lens[b] - 1;
        st[b] = mio::StepState{P, P, prompts[off[b] + P], 0};
        // as llm_begin: a full context ends the stream after n_ctx - len + 1 tokens
        budget[b] = std::min(max_tokens, D.n_ctx - prompt_lens[b] + 1);
        cf[b] = sample_cfg(m, sp, seeds[b], bt.tokens + (size_t)b * D.n_ctx, m->host_done_dev + 1 + b, P + budget[b]);
        cf[b].first_step = P;  // each stream's own history: the tokens it sampled
        __atomic_store_n(m->host_done + 1 + b, 0, __ATOMIC_SEQ_CST);
    }
    MIO_HIP_CHECK(hipMemcpyAsync(bt.st, st.data(), B * sizeof(mio::StepState), hipMemcpyHostToDevice, s));
    MIO_HIP_CHECK(hipMemcpyAsync(bt.cfg, cf.data(), B * sizeof(mio::SampleCfg), hipMemcpyHostToDevice, s));
    mio::launch_batch_embed(D, m->tok, step_pb(m), batch_bb(m), B, s);
    MIO_HIP_CHECK(hipGetLastError());
    // graphs of graph_steps() steps, at most kRunDepth queued ahead of the GPU; none issued once
    // every stream has stored its end token's host word or spent its step budget
    // (check_interval no longer paces this: r06)
    (void)check_interval;
    for (int issued = 0, k = 0; issued < max_tokens; ++k) {
        if ((rc = run_wait(m, k))) return rc;
        bool all = true;
        for (int b = 0; b < B && all; ++b)
            all = issued >= budget[b] || __atomic_load_n(m->host_done + 1 + b, __ATOMIC_ACQUIRE);
        if (all) break;
        const int n = std::min(graph_steps(), max_tokens - issued);
        if ((rc = run_batch(m, n, chain))) return rc;
        issued += n;
        if ((rc = run_mark(m, k))) return rc;
    }
    std::vector<mio::StepState> hs(B);
    MIO_HIP_CHECK(hipMemcpyAsync(hs.data(), bt.st, B * sizeof(mio::StepState), hipMemcpyDeviceToHost, s));
    MIO_HIP_CHECK(hipStreamSynchronize(s));
    std::vector<int32_t> ring(max_tokens);
    for (int b = 0; b < B; ++b) {
        const int P = prompt_lens[b] - 1;
        const int n = std::max(0, std::min(hs[b].step - P, max_tokens));
        if (n) MIO_HIP_CHECK(hipMemcpy(ring.data(), bt.tokens + (size_t)b * D.n_ctx + P, (size_t)n * 4,
                                       hipMemcpyDeviceToHost));
        int k = 0;
        while (k < n && ring[k] != eos0 && ring[k] != eos1) ++k;
        std::memcpy(out_tokens + (size_t)b * max_tokens, ring.data(), (size_t)k * 4);
        n_out[b] = k;
    }
    // the in-launch quantization's bounded wait (launch_mmq_q) raises this flag if a producer's
    // signal never came: an error instead of tokens computed from stale records
    int qflag = 0;
    MIO_HIP_CHECK(hipMemcpy(&qflag, m->pf.qcnt + mio::kQcntFlag, sizeof(int), hipMemcpyDeviceToHost));
    if (qflag) {
        MIO_HIP_CHECK(hipMemsetAsync(m->pf.qcnt + mio::kQcntFlag, 0, sizeof(int), m->d->stream));
        mio::set_error("llm_generate_batch: the in-launch quantization hand-off wait timed out");
        return MIO_ERR_HIP;
    }
    return MIO_OK;
}

// The launch structure of the batched step, observable: its kernel nodes as a captured graph.
extern "C" int mio_hip_llm_batch_step_launches(mio_hip_llm *m, int B, int *n) {
    MIO_REQUIRE(m && n, MIO_ERR_INVALID, "llm_batch_step_launches: null");
    // one step of B one-token streams first: the batch state for B, and the first step's eager
    // launches (the kernels' LDS attributes are set outside any capture, run_batch)
    std::vector<int32_t> prompts(B > 0 ? B : 1, 0), lens(B > 0 ? B : 1, 1), toks(B > 0 ? B : 1), cnt(B > 0 ? B : 1);
    std::vector<uint64_t> seeds(B > 0 ? B : 1, 1);
    if (int rc = mio_hip_llm_generate_batch(m, prompts.data(), lens.data(), B, 1, 0.0f, seeds.data(), -1, -1, -1, -1,
                                            1, toks.data(), cnt.data()))
        return rc;
    hipStream_t s = m->d->stream;
    MIO_HIP_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    issue_batch_steps(m, 1, false);
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamEndCapture(s, &g);
    size_t nn = 0;
    int kernels = 0;
    if (e == hipSuccess) e = hipGraphGetNodes(g, nullptr, &nn);
    std::vector<hipGraphNode_t> nodes(nn);
    if (e == hipSuccess && nn) e = hipGraphGetNodes(g, nodes.data(), &nn);
    for (size_t i = 0; i < nn && e == hipSuccess; ++i) {
        hipGraphNodeType ty;
        if ((e = hipGraphNodeGetType(nodes[i], &ty)) == hipSuccess && ty == hipGraphNodeTypeKernel) ++kernels;
    }
    if (g) hipGraphDestroy(g);
    MIO_HIP_CHECK(e);
    *n = kernels;
    return MIO_OK;
}
