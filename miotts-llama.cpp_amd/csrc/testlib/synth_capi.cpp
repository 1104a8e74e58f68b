// C-ABI: synthetic model files (no real GGUFs exist offline).
#include "common.h"
#include "synth.h"

extern "C" int mio_synth_codec_gguf(const char *path, int preset, uint64_t seed) {
    MIO_REQUIRE(path && preset >= 0 && preset <= 3, MIO_ERR_INVALID, "synth_codec: bad args");
    mio::SynthCodecCfg c = mio::synth_codec_preset(preset);
    c.seed = seed;
    MIO_REQUIRE(mio::synth_write_codec(path, c), MIO_ERR_IO, "synth_codec: cannot write %s", path);
    return MIO_OK;
}

extern "C" int mio_synth_voice_gguf(const char *path, uint64_t seed) {
    MIO_REQUIRE(path, MIO_ERR_INVALID, "synth_voice: null path");
    MIO_REQUIRE(mio::synth_write_voice(path, seed), MIO_ERR_IO, "synth_voice: cannot write %s", path);
    return MIO_OK;
}

extern "C" int mio_synth_llm_gguf(const char *path, int preset, uint64_t seed) {
    MIO_REQUIRE(path && preset >= 0 && preset < mio::kSynthLlmPresets, MIO_ERR_INVALID, "synth_llm: bad args");
    mio::SynthLlmCfg c = mio::synth_llm_preset(preset);
    c.seed = seed;
    MIO_REQUIRE(!mio::synth_llm_check(c), MIO_ERR_INVALID, "synth_llm: %s", mio::synth_llm_check(c));
    MIO_REQUIRE(mio::synth_write_llm(path, c), MIO_ERR_IO, "synth_llm: cannot write %s", path);
    return MIO_OK;
}

extern "C" int mio_synth_llm_gguf_as(const char *path, int preset, int qtype, uint64_t seed) {
    MIO_REQUIRE(path && preset >= 0 && preset < mio::kSynthLlmPresets, MIO_ERR_INVALID, "synth_llm_as: bad args");
    MIO_REQUIRE(mio::synth_llm_qtype_known(qtype), MIO_ERR_INVALID, "synth_llm_as: unknown recipe %d", qtype);
    mio::SynthLlmCfg c = mio::synth_llm_preset(preset);
    c.qtype = qtype;
    c.seed = seed;
    MIO_REQUIRE(!mio::synth_llm_check(c), MIO_ERR_INVALID, "synth_llm_as: %s", mio::synth_llm_check(c));
    MIO_REQUIRE(mio::synth_write_llm(path, c), MIO_ERR_IO, "synth_llm_as: cannot write %s", path);
    return MIO_OK;
}

extern "C" int mio_synth_llm_gguf_shape(const char *path, int preset, int qtype, uint64_t seed, int n_embd,
                                        int n_layer, int n_head, int n_head_kv, int n_ff) {
    MIO_REQUIRE(path && preset >= 0 && preset < mio::kSynthLlmPresets, MIO_ERR_INVALID, "synth_llm_shape: bad args");
    MIO_REQUIRE(mio::synth_llm_qtype_known(qtype), MIO_ERR_INVALID, "synth_llm_shape: unknown recipe %d", qtype);
    MIO_REQUIRE(n_embd >= 0 && n_layer >= 0 && n_head >= 0 && n_head_kv >= 0 && n_ff >= 0, MIO_ERR_INVALID,
                "synth_llm_shape: negative size");
    mio::SynthLlmCfg c = mio::synth_llm_preset(preset);
    c.qtype = qtype;
    c.seed = seed;
    if (n_embd) c.n_embd = n_embd;
    if (n_layer) c.n_layer = n_layer;
    if (n_head) c.n_head = n_head;
    if (n_head_kv) c.n_head_kv = n_head_kv;
    if (n_ff) c.n_ff = n_ff;
    // every row length is whole 32-element blocks, and the kv heads divide the heads
    MIO_REQUIRE(c.n_embd % 32 == 0 && c.n_ff % 32 == 0 && c.n_head_kv <= c.n_head && c.n_head % c.n_head_kv == 0,
                MIO_ERR_INVALID, "synth_llm_shape: n_embd %d / n_ff %d must be multiples of 32, heads %d / %d", c.n_embd,
                c.n_ff, c.n_head, c.n_head_kv);
    MIO_REQUIRE(!mio::synth_llm_check(c), MIO_ERR_INVALID, "synth_llm_shape: %s", mio::synth_llm_check(c));
    MIO_REQUIRE(mio::synth_write_llm(path, c), MIO_ERR_IO, "synth_llm_shape: cannot write %s", path);
    return MIO_OK;
}
