// Batched decode engine of the LLM runner (see llm.h, llm_model.h): independent utterances
// decoded together on the multi-token layers (csrc/hip/llm_prefill.hip), one weight pass per
// step for all of them. One engine, the utterance queue (queue_run), behind both entries:
// mio_hip_llm_generate_batch is the queue with a slot for every utterance.
#include <algorithm>
#include <climits>
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
    bt.ppos = (int *)al((size_t)B * D.n_ctx * 4);
    bt.pseq = (int *)al((size_t)B * D.n_ctx * 4);
    bt.ptok = (int *)al((size_t)B * D.n_ctx * 4);
    bt.ring = m->buf.ring ? (float *)al(B * batch_seq_ring(m) * 4) : nullptr;
    if (!bt.kc || !bt.vc || !bt.st || !bt.cfg || !bt.logits || !bt.smp || !bt.ppos || !bt.pseq || !bt.ptok ||
        (m->buf.ring && !bt.ring)) {
        for (void *p : bt.allocs) hipFree(p);
        bt.allocs.clear();
        mio::set_error("llm batched decode: device allocation for %d streams failed", B);
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

// What one call (either entry) owns on the device, and its per-utterance end-token words. One
// word per utterance, not per slot: a slot whose budget the host counts as spent may
// still have its last steps queued, and one of them can store an end-token word after the host
// has admitted the next utterance there; that store must not land in the new utterance's word.
// The buffers are sized by the call (N, its prompts, its budgets), so they are allocated and
// released per call: four allocations and frees, each a device-wide synchronise, once per call
// and never per refill.
struct QueueCall {
    mio::Scratch<int> tokens, out;
    mio::Scratch<mio::QueueUtt> utt;
    mio::Pinned<int> done;
    int *done_dev = nullptr;
};

// The queue itself (arguments checked, device bound). Work it queued may still be running when
// it returns an error: the caller drains the stream before the buffers go.
int queue_run(const char *who, mio_hip_llm *m, const int32_t *prompts, const int32_t *prompt_lens,
              const std::vector<int> &off, int N, int S, int max_tokens, const mio::SamplingParams &sp,
              const uint64_t *seeds, QueueCall &qc, int32_t *out_tokens, int32_t *n_out, mio_llm_queue_stats *stats) {
    const mio::LlmDims &D = m->dims;
    auto &bt = m->bt;
    hipStream_t s = m->d->stream;
    int rc;
    // one upload: every prompt, and per utterance where its prompt lies, its seed, its budget
    // (as llm_begin: a full context ends it after n_ctx - len + 1 tokens) and its output region
    std::vector<mio::QueueUtt> utt(N);
    size_t out_ints = (size_t)D.n_ctx;
    for (int u = 0; u < N; ++u) {
        const int budget = std::min(max_tokens, D.n_ctx - prompt_lens[u] + 1);
        utt[u] = mio::QueueUtt{off[u], prompt_lens[u] - 1, budget, (int)out_ints, (uint32_t)seeds[u],
                               (uint32_t)(seeds[u] >> 32)};
        out_ints += (size_t)budget;
    }
    MIO_REQUIRE(out_ints < ((size_t)1 << 31), MIO_ERR_INVALID, "%s: %d utterances x their budgets overflow", who, N);
    MIO_HIP_CHECK(hipMalloc((void **)qc.tokens.put(), (size_t)off[N] * 4));
    MIO_HIP_CHECK(hipMalloc((void **)qc.utt.put(), (size_t)N * sizeof(mio::QueueUtt)));
    MIO_HIP_CHECK(hipMalloc((void **)qc.out.put(), out_ints * 4));
    // coherent, as the handle's own end-token words: the sampler's system-scope store must be
    // visible to the host while the graphs still run
    MIO_HIP_CHECK(hipHostMalloc((void **)qc.done.put(), (size_t)N * sizeof(int),
                                hipHostMallocMapped | hipHostMallocCoherent));
    MIO_HIP_CHECK(hipHostGetDevicePointer((void **)&qc.done_dev, qc.done.get(), 0));
    std::memset(qc.done.get(), 0, (size_t)N * sizeof(int));
    MIO_HIP_CHECK(hipMemcpyAsync(qc.tokens.get(), prompts, (size_t)off[N] * 4, hipMemcpyHostToDevice, s));
    MIO_HIP_CHECK(
        hipMemcpyAsync(qc.utt.get(), utt.data(), (size_t)N * sizeof(mio::QueueUtt), hipMemcpyHostToDevice, s));
    // -1 everywhere: what an utterance did not sample stays -1 (token ids are >= 0)
    MIO_HIP_CHECK(hipMemsetAsync(qc.out.get(), 0xFF, out_ints * 4, s));
    const mio::QueueBuffers qb{qc.tokens.get(), qc.utt.get(), qc.out.get(), qc.done_dev, bt.ptok, bt.ppos, bt.pseq};
    const bool chain = chain_on(sp);
    const mio::SampleCfg base = sample_cfg(m, sp, 0, nullptr, nullptr, 0);

    // slot b decodes utterance cur[b] (-1: none yet), admitted when `steps` was start[b]
    std::vector<int> cur(S, -1), start(S, 0);
    int steps = 0, next = 0, refills = 0, chunks = 0;
    bool fin[mio::kBatchMax];
    // graph k's event is run_ev[k % kRunDepth]: the one graph k - kRunDepth recorded, which is the
    // graph to wait for before k is issued (run_wait / run_mark keep one event per graph, which
    // here would grow with N)
    for (int k = 0;;) {
        if (k >= kRunDepth) MIO_HIP_CHECK(hipEventSynchronize(m->run_ev[k % kRunDepth]));
        // one look at every slot per boundary: the GPU is still running the graph queued last, so
        // an end-token word can be stored at any moment, and everything below must decide from
        // the same picture (a word read again later could end the loop with utterances waiting)
        for (int b = 0; b < S; ++b)
            fin[b] = cur[b] < 0 || steps - start[b] >= utt[cur[b]].budget ||
                     __atomic_load_n(qc.done.get() + cur[b], __ATOMIC_ACQUIRE);
        // admissions of this graph boundary, in slot order, on the runner's stream: behind every
        // step already queued, so the slot's old utterance is frozen when they run
        mio::QueueRefill r{};
        std::vector<int> fpos;  // the position of every token of the flattened lists (host copy)
        for (int b = 0; b < S && next < N; ++b) {
            if (!fin[b]) continue;
            if (cur[b] >= 0) ++refills;
            const int u = next++;
            r.slot[r.n] = b, r.utt[r.n] = u, r.flat[r.n] = (int)fpos.size(), ++r.n;
            for (int p = 0; p < utt[u].P; ++p) fpos.push_back(p);
            cur[b] = u, start[b] = steps, fin[b] = false;  // budget >= 1, its word is still 0
            if (stats && stats->slot_of) stats->slot_of[u] = b;
            if (stats && stats->start_step) stats->start_step[u] = steps;
        }
        if (r.n) {
            mio::launch_queue_refill(step_pb(m), qb, r, s);
            const int nf = (int)fpos.size();
            for (int c0 = 0; c0 < nf; c0 += mio::kPrefillB, ++chunks) {
                const int nt = std::min(nf - c0, mio::kPrefillB);
                const int pmax = *std::max_element(fpos.begin() + c0, fpos.begin() + c0 + nt);
                mio::PrefillBuffers pb = batch_pb(m, bt.ppos + c0, 1, bt.pseq + c0);
                pb.tokens = bt.ptok;
                mio::launch_prefill_chunk(D, m->layers.data(), m->n_layer, bt.kc, bt.vc, m->tok, pb, c0, nt,
                                          pmax / mio::kAttChunk + 1, s);
            }
            mio::launch_queue_admit(D, m->tok, step_pb(m), batch_bb(m), bt.cfg, base, qb, r, S, s);
            MIO_HIP_CHECK(hipGetLastError());
        }
        // steps to the next boundary: a graph's worth, or what the longest live budget still takes
        int left = 0;
        for (int b = 0; b < S; ++b)
            if (!fin[b]) left = std::max(left, utt[cur[b]].budget - (steps - start[b]));
        if (left == 0) {
            // every slot is finished; with utterances waiting they were all admitted above and are
            // live, so this is the end only when the queue is empty too
            if (next >= N) break;
            continue;
        }
        const int n = std::min(graph_steps(), left);
        if ((rc = run_batch(m, n, chain))) return rc;
        steps += n;
        if ((rc = run_mark(m, k % kRunDepth))) return rc;
        ++k;
    }
    std::vector<int32_t> out(out_ints);
    MIO_HIP_CHECK(hipMemcpyAsync(out.data(), qc.out.get(), out_ints * 4, hipMemcpyDeviceToHost, s));
    // every slot is frozen now, and its SampleCfg still points at this call's output region and
    // end-token word, which go when the call returns. The next call admits into every slot it
    // runs, which writes that slot's cfg first; zeroed, the slots stay frozen (max_steps 0) and
    // name no freed memory whoever comes
    MIO_HIP_CHECK(hipMemsetAsync(bt.cfg, 0, (size_t)S * sizeof(mio::SampleCfg), s));
    MIO_HIP_CHECK(hipStreamSynchronize(s));
    long live = 0;
    for (int u = 0; u < N; ++u) {
        const int32_t *t = out.data() + utt[u].out_off;
        int n = 0, k = 0;
        while (n < utt[u].budget && t[n] >= 0) ++n;  // sampled, the end token included
        while (k < n && t[k] != sp.eos0 && t[k] != sp.eos1) ++k;
        std::memcpy(out_tokens + (size_t)u * max_tokens, t, (size_t)k * 4);
        n_out[u] = k;
        live += n;
    }
    if (stats) {
        stats->steps = steps, stats->live_slot_steps = (int32_t)live;
        stats->refills = refills, stats->prefill_chunks = chunks;
    }
    return MIO_OK;
}

// What both entries check before anything touches the device (who: the entry's name, for the
// messages; slots: the streams the batched step would run, checked as the caller gave them).
// off[u] = where utterance u's prompt starts in `prompts`, off[N] = their total.
int check_call(const char *who, const mio_hip_llm *m, const int32_t *prompts, const int32_t *prompt_lens, int N,
               int slots, int max_tokens, const uint64_t *seeds, const int32_t *out_tokens, const int32_t *n_out,
               std::vector<int> &off) {
    MIO_REQUIRE(m && prompts && prompt_lens && seeds && out_tokens && n_out && max_tokens >= 1, MIO_ERR_INVALID,
                "%s: bad args", who);
    MIO_REQUIRE(mio::batch_supported(m->dims, slots, m->lm.type), MIO_ERR_UNSUPPORTED,
                "%s: %d streams not supported (1..%d, lm_head LDS)", who, slots, mio::kBatchMax);
    MIO_REQUIRE(m->bf16_mt(), MIO_ERR_UNSUPPORTED,
                "%s: BF16 weights mixed with quantized ones run on the single-stream decode only "
                "(mio_hip_llm_generate)", who);
    const mio::LlmDims &D = m->dims;
    off.assign(N + 1, 0);
    for (int u = 0; u < N; ++u) {
        MIO_REQUIRE(prompt_lens[u] >= 1 && prompt_lens[u] <= D.n_ctx, MIO_ERR_INVALID,
                    "%s: utterance %d: %d prompt tokens exceed n_ctx %d", who, u, prompt_lens[u], D.n_ctx);
        MIO_REQUIRE(off[u] <= INT32_MAX - prompt_lens[u], MIO_ERR_INVALID, "%s: too many prompt tokens", who);
        off[u + 1] = off[u] + prompt_lens[u];
    }
    for (int i = 0; i < off[N]; ++i)
        MIO_REQUIRE(prompts[i] >= 0 && prompts[i] < D.n_vocab, MIO_ERR_INVALID, "%s: token %d out of vocab", who,
                    prompts[i]);
    return MIO_OK;
}

// A call's sampler: the handle's chain knobs (mio_hip_llm_set_sampling), shared by every utterance,
// and the call's own temperature, allowed range and end tokens.
mio::SamplingParams call_sampling(const mio_hip_llm *m, float temperature, int32_t allow_lo, int32_t allow_hi,
                                  int32_t eos0, int32_t eos1) {
    mio::SamplingParams sp = m->sampling;
    sp.temperature = temperature, sp.allow_lo = allow_lo, sp.allow_hi = allow_hi, sp.eos0 = eos0, sp.eos1 = eos1;
    return sp;
}

// End of a call: the in-launch quantization's bounded wait (launch_mmq_q) raises this flag if a
// producer's signal never came: an error instead of tokens computed from stale records.
int check_quant_wait(mio_hip_llm *m, const char *who) {
    int qflag = 0;
    MIO_HIP_CHECK(hipMemcpy(&qflag, m->pf.qcnt + mio::kQcntFlag, sizeof(int), hipMemcpyDeviceToHost));
    if (qflag) {
        MIO_HIP_CHECK(hipMemsetAsync(m->pf.qcnt + mio::kQcntFlag, 0, sizeof(int), m->d->stream));
        mio::set_error("%s: the in-launch quantization hand-off wait timed out", who);
        return MIO_ERR_HIP;
    }
    return MIO_OK;
}

// Both entries: N utterances on min(slots, N) streams of the batched decode.
int generate_on_queue(const char *who, mio_hip_llm *m, const int32_t *prompts, const int32_t *prompt_lens, int N,
                      int slots, int max_tokens, float temperature, const uint64_t *seeds, int32_t allow_lo,
                      int32_t allow_hi, int32_t eos0, int32_t eos1, int32_t *out_tokens, int32_t *n_out,
                      mio_llm_queue_stats *stats) {
    std::vector<int> off;
    int rc = check_call(who, m, prompts, prompt_lens, N, slots, max_tokens, seeds, out_tokens, n_out, off);
    if (rc || (rc = mio::bind(m->d)) || (rc = batch_ensure(m, std::min(slots, N))) || (rc = reset_tickets(m)))
        return rc;
    const mio::SamplingParams sp = call_sampling(m, temperature, allow_lo, allow_hi, eos0, eos1);
    QueueCall qc;
    if ((rc = queue_run(who, m, prompts, prompt_lens, off, N, m->bt.B, max_tokens, sp, seeds, qc, out_tokens, n_out,
                        stats))) {
        (void)hipStreamSynchronize(m->d->stream);  // nothing queued outlives the call's buffers
        return rc;
    }
    return check_quant_wait(m, who);
}

}  // namespace

// An utterance queue on the batched decode: N utterances on min(slots, N) streams, the next one
// admitted into a slot at the first step-graph boundary after the slot's utterance has ended
// ("Utterance queue"). Each utterance's tokens equal a single-stream generate with its
// seed: the same kernels' arithmetic per token, the same sampler noise. (The reference runs
// utterances one after another, one llama_context each: test-to-speech.cpp:94-199 per call.)
extern "C" int mio_hip_llm_generate_queue(mio_hip_llm *m, const int32_t *prompts, const int32_t *prompt_lens, int N,
                                          int slots, int max_tokens, float temperature, const uint64_t *seeds,
                                          int32_t allow_lo, int32_t allow_hi, int32_t eos0, int32_t eos1,
                                          int32_t *out_tokens, int32_t *n_out, mio_llm_queue_stats *stats) {
    MIO_REQUIRE(N >= 1, MIO_ERR_INVALID, "llm_generate_queue: bad args");
    return generate_on_queue("llm_generate_queue", m, prompts, prompt_lens, N, slots, max_tokens, temperature, seeds,
                             allow_lo, allow_hi, eos0, eos1, out_tokens, n_out, stats);
}

// B utterances decoded together: the queue with as many slots as utterances, so all of them are
// admitted at its first boundary and nothing is refilled. B itself is what is checked as the
// slot count: more than the batched step takes is refused, never run on fewer slots.
// check_interval is unused (the end-token words pace the call).
extern "C" int mio_hip_llm_generate_batch(mio_hip_llm *m, const int32_t *prompts, const int32_t *prompt_lens, int B,
                                          int max_tokens, float temperature, const uint64_t *seeds,
                                          int32_t allow_lo, int32_t allow_hi, int32_t eos0, int32_t eos1,
                                          int32_t check_interval, int32_t *out_tokens, int32_t *n_out) {
    (void)check_interval;
    return generate_on_queue("llm_generate_batch", m, prompts, prompt_lens, B, B, max_tokens, temperature, seeds,
                             allow_lo, allow_hi, eos0, eos1, out_tokens, n_out, nullptr);
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
