// LLM decode runner on one MI355X (replaces the llama.cpp context used by
// TestToSpeech::run_llm, test-to-speech.cpp:94-199 / :435-614).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

struct mio_hip_device;
struct mio_hip_llm;

namespace mio {

struct LlmInfo {
    int n_vocab, n_embd, n_layer, n_head, n_kv, head_dim, n_ff, n_ctx;
};

struct SamplingParams {
    float temperature = 0.8f;
    uint64_t seed = 42;      // llama_sampler_init_dist(42), test-to-speech.cpp:130
    int allow_lo = 0, allow_hi = -1;  // restrict sampling to [lo, hi) (-1 = n_vocab)
    int eos0 = -1, eos1 = -1;
    // the sampler chain (include/mio_hip.h mio_sampling; these defaults are the neutral values:
    // no chain launch)
    int top_k = 0;
    float top_p = 1.0f, min_p = 0.0f, repeat_penalty = 1.0f, frequency_penalty = 0.0f, presence_penalty = 0.0f;
    int repeat_last_n = 64;
};

// Incremental generation on the device: begin() seeds the prompt, run() enqueues decode
// steps (one hipGraph replay each), poll() syncs and returns the tokens produced so far.
int llm_begin(mio_hip_llm *m, const int32_t *prompt, int n_prompt, int max_new,
              const SamplingParams &sp);
int llm_run(mio_hip_llm *m, int n_steps);
// Every remaining step, stopping (at step-graph granularity) once the device has flagged an
// end token to the host; then the flush sampler and a snapshot for llm_poll.
int llm_run_to_end(mio_hip_llm *m);
int llm_graph_steps();
// Copies generated tokens [0, *n_out) and reports whether an end token was sampled.
int llm_poll(mio_hip_llm *m, std::vector<int32_t> &out, bool *done);
LlmInfo llm_info(const mio_hip_llm *m);
uint64_t llm_step_weight_bytes(const mio_hip_llm *m);

// Parity-test entry points of the attention launches (exported as C by the test-support
// library, include/mio_hip_test.h; no product path calls them).
// F16 rows k, v [n_kv][n_pos][head_dim] into cache positions [p0, p0 + n_pos) of layer il (the
// inverse of mio_hip_llm_kv_rows).
int llm_set_kv_rows(mio_hip_llm *m, int il, int p0, int n_pos, const uint16_t *k, const uint16_t *v);
// One attention launch of layer il at position pos on the raw q|k|v row qkv[(H + 2 Hkv) hd]:
// which = 1 (k_attention) or 10 (k_att_o); att[H hd] receives LlmBuffers.att. Leaves the decode
// state at pos and cache row pos written.
int llm_debug_attention(mio_hip_llm *m, int il, int pos, int which, const float *qkv, float *att);
// words[3 n_kv]: per kv head the q row counter, the q|k|v row counter and the chunk arrival word of
// the fused attention launches (0 between steps); reset != 0: after reset_tickets.
int llm_handoff_words(mio_hip_llm *m, int reset, int32_t *words);
// One sampler chain launch (k_sample_chain) + the flush sampler on the injected row
// logits[n_vocab], with history[n_history] as the tokens sampled before `step` and sp's
// temperature, seed, window and chain knobs: the token, the kept count, the id at the cut and
// (not null) the penalised row.
int llm_debug_sample_chain(mio_hip_llm *m, const float *logits, const int32_t *history, int n_history,
                           const SamplingParams &sp, int step, int32_t *token, int32_t *kept, int32_t *cut_id,
                           float *penalised);

}  // namespace mio
