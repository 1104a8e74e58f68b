// The LLM runner's model object and the helpers its translation units share (private to
// csrc/host): llm_load.cpp (GGUF -> HBM), llm.cpp (decode runtime), llm_batch.cpp (batched
// engine), llm_diag.cpp (parity-test entry points and profiling diagnostics).
#pragma once

#include <cstdlib>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "common.h"
#include "hip_own.h"
#include "llm.h"
#include "llm_kernels.h"

#pragma GCC visibility push(hidden)
// Host -> HBM weight upload: every matrix is re-laid out (to_split) from the mmapped GGUF
// straight into one of two pinned staging buffers while the other buffer's DMA copy runs
// (hipMemcpyAsync on a load stream), instead of a pageable vector + a synchronous copy.
struct Stager {
    hipStream_t s = nullptr;
    void *buf[2] = {nullptr, nullptr};
    size_t cap[2] = {0, 0};
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool used[2] = {false, false};
    int cur = 0;

    bool init();
    uint8_t *acquire(size_t bytes);  // a staging buffer of >= bytes whose previous copy has finished
    bool submit(void *dst, size_t bytes);
    bool finish();
    ~Stager();
};
#pragma GCC visibility pop

struct mio_hip_llm {
    mio_hip_device *d = nullptr;
    mio::LlmDims dims{};
    int n_layer = 0;
    std::vector<mio::LayerW> layers;
    // per layer: ffn_gate is stored as a type that runs repacked to Q8_0 (Q5_0 / Q4_0), not as Q8_0
    std::vector<char> gate_repacked;
    mio::QMat tok{}, lm{};
    float *out_norm = nullptr;
    _Float16 *kc = nullptr, *vc = nullptr;
    // what every launch_step_kernel of this model gets (built once, at the end of the load)
    mio::StepCtx step{};
    const mio::StepCtx &ctx() const { return step; }
    mio::LlmBuffers buf{};
    int *d_tokens = nullptr, *d_force = nullptr, *d_prompt = nullptr;
    mio::PrefillBuffers pf{};  // batched prompt prefill (kPrefillB tokens per chunk)
    int *d_iota = nullptr;     // 0, 1, ..., n_ctx - 1 (prefill positions; batch stream ids)
    // batched decode on B streams (mio_hip_llm_generate_batch / _queue), allocated on first use
    struct Batch {
        int B = 0;
        _Float16 *kc = nullptr, *vc = nullptr;  // [B][layer][kv head][n_ctx][hd]
        mio::StepState *st = nullptr;
        mio::SampleCfg *cfg = nullptr;
        float *logits = nullptr, *smp = nullptr;
        int *ppos = nullptr, *pseq = nullptr, *ptok = nullptr;  // flattened prompt prefill lists
        float *ring = nullptr;  // lfm2: [B][n_layer][kConvSlots][n_embd] short-conv rings
        mio::GraphExec graph, graph_n;
        mio::GraphExec graph_c, graph_cn;  // with the sampler chain launch
        std::vector<void *> allocs;
    } bt;
    int max_steps = 0;
    std::vector<void *> allocs;
    uint64_t weight_bytes = 0;
    // BF16 matrices: the multi-token engine runs them on its streaming dot engine with bf16
    // act records (rec_k) when every matrix is BF16 (attention and lfm2 short-conv layers
    // alike); a BF16 matrix beside an int8 one (bf16_mt false) has the prompt prefilled as
    // forced decode steps and batched decode refused
    bool bf16 = false, int8 = false, has_conv = false;
    bool bf16_mt() const { return !bf16 || !int8; }
    // all quantized matrices live in one arena, in the order a step streams them
    uint8_t *arena = nullptr;
    std::map<std::string, size_t> arena_off;

    // decode-step graphs, captured once (the sampling config is device-resident):
    // one step, and graph_steps() steps back to back (fewer graph launches per token)
    mio::GraphExec graph, graph_n;
    // the same pair with the sampler chain launch in every step (captured when a generate first
    // runs with a chain knob on; the pair above is never re-captured)
    mio::GraphExec graph_c, graph_cn;
    // the chain knobs later generates run with (mio_hip_llm_set_sampling; the other fields are
    // unused), and whether the generate in progress has the chain launch in its steps
    mio::SamplingParams sampling;
    bool chain = false;
    // prompt prefills replayed as graphs, by prompt length (the first prefill of a length runs
    // eagerly and is captured: ~280 launches that eager issue makes host-bound)
    std::map<int, mio::GraphExec> prefill_graphs;
    std::map<int, int> prefill_seen;  // eager prefills per prompt length (capture on the second)
    mio::SampleCfg *d_cfg = nullptr;
    float *d_layers = nullptr;  // mio_hip_llm_eval_layers' residual snapshots (parity tests)
    // generation state
    int n_prompt = 0, max_new = 0, steps_total = 0, steps_issued = 0;
    // weight passes the last prefill / generate spent on prompt positions [0, n - 1)
    // (mio_hip_llm_prompt_chunks)
    int prompt_chunks = 0;
    mio::SampleCfg cfg{};
    double load_ms = 0.0;  // wall time of mio_hip_llm_load (GGUF mmap -> HBM arena)
    std::unique_ptr<Stager> stager;  // weight upload staging (load only)
    // token-ring snapshots (pinned host mirrors of the state and the ring): llm_run enqueues
    // one behind its steps, llm_poll waits for the OLDEST one, so a caller can enqueue the next
    // interval before it waits for the previous (the GPU never idles at a poll)
    struct Snap {
        mio::Event ev;
        mio::Pinned<mio::StepState> st;
        mio::Pinned<int> tok;
        int hi = 0, issued = 0;
    };
    static constexpr int kSnaps = 2;
    Snap snaps[kSnaps];
    int snap_head = 0, snap_n = 0;  // oldest outstanding snapshot, number outstanding
    // steps run after the end token of the last generate (mio_hip_llm_tail): slot of the
    // snapshot whose poll found it (-1: none), steps issued in total after it, and the GPU
    // time of the whole intervals queued behind that snapshot
    int eos_snap = -1, tail_steps = 0, tail_timed_steps = 0;
    float tail_ms = 0.0f;
    // the end-token word the single-stream decode's sampler stores to host memory (pinned, mapped;
    // a batched call has words of its own, one per utterance), so the host stops enqueuing steps
    // without a blocking poll; and one event per step graph of the running generate (flow control: at most
    // kRunDepth graphs queued ahead of the GPU; the tail timing)
    mio::Pinned<int> host_done;
    int *host_done_dev = nullptr;
    std::vector<mio::Event> run_ev;
    int run_base = 0, run_graphs = 0;  // steps issued before the first graph; graphs issued

    // the device is made current before anything is released; the owners above then release
    // their handles (graphs, events, pinned memory, the stager) in reverse order
    ~mio_hip_llm() {
        if (d) hipSetDevice(d->dev);
        for (void *p : bt.allocs) hipFree(p);
        for (void *p : allocs) hipFree(p);
    }
};

#pragma GCC visibility push(hidden)

// llm.cpp: the step plan
int graph_steps();  // steps per replayed step graph (MIO_GRAPH_STEPS)
bool no_graph();    // MIO_NO_GRAPH=1: every launch eager
bool fuse_att_o(const mio_hip_llm *m);
bool fuse_layer_att(const mio_hip_llm *m, int il);
bool fuse_ffn(const mio_hip_llm *m, int il);
// can this model run launch `kind` on layer il (kLmHead / kSample: on any)
bool kind_in_layer(const mio_hip_llm *m, mio::StepKind kind, int il);
constexpr int kLayerKindsMax = 5;
int layer_kinds(const mio_hip_llm *m, int il, mio::StepKind *w);  // layer il's launches in order; the count
std::vector<mio::StepKind> step_kinds(const mio_hip_llm *m);      // every launch of a step in order
// llm.cpp: the decode runtime
int issue_step(mio_hip_llm *m, unsigned long long *tl = nullptr, bool chain = false);
int flush_sample(mio_hip_llm *m);
int ensure_graph(mio_hip_llm *m, bool chain = false);
bool chain_on(const mio::SamplingParams &sp);                     // a chain knob is off its neutral value
int check_chain(const mio::SamplingParams &sp, const char *who);  // MIO_ERR_INVALID for values no chain takes
int put_cfg(mio_hip_llm *m, mio::SampleCfg c);
mio::SampleCfg greedy_cfg(const mio_hip_llm *m);
mio::SampleCfg sample_cfg(const mio_hip_llm *m, const mio::SamplingParams &sp, uint64_t seed, int *out_tokens,
                          int *host_done, int max_steps);
int set_state(mio_hip_llm *m, int pos, int token, int step = 0);
int reset_tickets(mio_hip_llm *m);
int reset_rdy(mio_hip_llm *m, hipStream_t s);
int check_handoff(mio_hip_llm *m);
int prefill(mio_hip_llm *m, int n);
// Flow control of a generate's step graphs: at most kRunDepth queued ahead of the GPU.
// run_wait(k) waits, before graph k is issued, for the graph kRunDepth back; run_mark(k)
// records graph k's event behind it (growing run_ev).
constexpr int kRunDepth = 2;
int run_wait(mio_hip_llm *m, int k);
int run_mark(mio_hip_llm *m, int k);

#pragma GCC visibility pop
